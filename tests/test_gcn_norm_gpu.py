"""GCN-normalised aggregation: ops.gcn_norm and ops.gcn_aggregate (euler_gpu_gcn_norm,
euler_gpu_gather_reduce_norm_t).

Contract (include/euler_gpu.h):
A. norm tables: the bits of numpy's float32(1) / sqrt(float32(deg)), 0 at degree 0; an edge counts
   iff both keys are in range.
B. forward - fp32: the bits of the restatement tests/gcn_norm_ref.py and of
   gather_scatter(op, x, src, dst, n, edge_weight=norm_dst[dst] * norm_src[src]); storage dtype S:
   f_S(x, out_dtype=fp32) has the bits of f_fp32(x.float()), f_S(..., out_dtype=S) those after .to(S).
C. epilogue: the bits of agg * a + root * b in torch fp32, rounded once to the output type.
D. grad_x and grad_root have the bits of the composition's gradients under torch autograd.
E. against float64 with exact integer degrees and w = 1 / sqrt(deg_i * deg_j):
   |out - ref| <= gamma_(n + 5) * sum_p |w_p x_p|, n the segment length, gamma_k = k u / (1 - k u),
   u = 2^-24 - two roundings per norm, one for their product, one for the message, n - 1 for the
   sum; mean adds one; a 16-bit output half an ulp at the reference value.  Derived: no margin.
Inputs are finite with |x| <= 4."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from test_half_mp_gpu import DIMS
import gcn_norm_ref as ref

pytestmark = pytest.mark.gpu

OPS = ["add", "mean"]
U = 2.0 ** -24
ROWS, SIZE, COUNT = 100, 40, 5
E = SIZE * COUNT


def _dtypes(torch):
    return [torch.float32, torch.bfloat16, torch.float16]


def bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same(got, want):
    import torch
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(bits(got), bits(want))


def same_np(torch, got, want):
    return same(got, torch.from_numpy(np.ascontiguousarray(want, np.float32)).cuda())


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


@pytest.fixture(scope="module")
def gen(torch_cuda):
    g = torch_cuda.Generator(device="cuda")
    g.manual_seed(2222)
    return g


@pytest.fixture(scope="module")
def block(torch_cuda, gen):
    """The destinations of one small block in its four forms (each its own edge list), built once:
    name -> dict(src, dst keys as every op sees them, kwargs of the segment forms)"""
    torch = torch_cuda
    src = torch.randint(0, ROWS, (E,), generator=gen, device="cuda", dtype=torch.int32)
    si = torch.randint(0, SIZE + 5, (E,), generator=gen, device="cuda", dtype=torch.int32)   # some keys >= size
    si[(si % 7) == 3] += 1                                   # destinations 3, 10, 17, ... stay empty
    si[::31] = -1
    lens = torch.randint(0, 11, (SIZE,), generator=gen, device="cuda")
    lens[::9] = 0
    seg_ptr = torch.zeros(SIZE + 1, dtype=torch.int64, device="cuda")
    seg_ptr[1:] = torch.cumsum(lens, 0)
    ep = int(seg_ptr[-1])
    src_p = torch.randint(0, ROWS, (ep,), generator=gen, device="cuda", dtype=torch.int32)
    ar = torch.arange(SIZE, device="cuda", dtype=torch.int32)
    return {
        "unsorted": dict(src=src, dst=si, kw={}),
        "sorted": dict(src=src, dst=torch.sort(si).values, kw={}),
        "seg_ptr": dict(src=src_p, dst=torch.repeat_interleave(ar, lens), kw=dict(seg_ptr=seg_ptr)),
        "count": dict(src=src, dst=ar.repeat_interleave(COUNT), kw=dict(count=COUNT)),
    }


def edges_of(form):
    """the edge_index argument of a form: (dst, src) for keys, the source column for segments"""
    return form["src"] if form["kw"] else (form["dst"], form["src"])


def edge_weight(torch, norm, dst, src, n_dst):
    """norm_dst[dst] * norm_src[src] per edge, fp32; an out-of-range destination (which every reduce
    leaves out) reads entry 0"""
    d = dst.long()
    d = torch.where((d >= 0) & (d < n_dst), d, torch.zeros_like(d))
    return norm[0][d] * norm[1][src.long()]


def test_norm_tables(EA, torch_cuda):
    """destination k has degree k for k = 0 .. 300, destination 301 and source 0 are hubs of degree
    70 000; shuffled, with keys -1, size and 2^31 - 1 mixed in on both sides.  An uncorrected
    square root (1 ulp) fails here."""
    torch = torch_cuda
    rng = np.random.default_rng(7)
    n_dst, n_src, hub = 302, 500, 70000
    dst = np.concatenate([np.repeat(np.arange(301), np.arange(301)), np.full(hub, 301)])
    src = np.concatenate([rng.integers(1, n_src - 1, dst.size - hub), np.zeros(hub, np.int64)])
    bad = np.array([-1, n_dst, 2 ** 31 - 1, 5, 6, 7, -1, 2 ** 31 - 1], np.int64)
    bad_src = np.array([3, 4, 5, -1, n_src, 2 ** 31 - 1, -1, n_src], np.int64)
    dst, src = np.concatenate([dst, np.tile(bad, 50)]), np.concatenate([src, np.tile(bad_src, 50)])
    order = rng.permutation(dst.size)
    dst, src = dst[order].astype(np.int32), src[order].astype(np.int32)
    dd, ds = ref.degrees(dst, src, n_dst, n_src)
    assert dd[:301].tolist() == list(range(301)) and dd[301] == hub and ds[0] == hub and ds[n_src - 1] == 0
    want_d, want_s = ref.gcn_norm(dst, src, n_dst, n_src)
    ei = torch.from_numpy(np.stack([dst, src])).cuda()
    nd, ns = EA.ops.gcn_norm(ei, (n_dst, n_src))
    assert same_np(torch, nd, want_d) and same_np(torch, ns, want_s)
    assert float(nd[0]) == 0.0 and float(ns[n_src - 1]) == 0.0 and bool(torch.isfinite(nd).all())
    nd2, ns2 = EA.ops.gcn_norm((ei[0], ei[1].long()), (n_dst, n_src))      # a pair; run to run
    assert same(nd2, nd) and same(ns2, ns)
    # an empty block, and tables of length 0
    e0 = torch.zeros((2, 0), dtype=torch.int32, device="cuda")
    z = EA.ops.gcn_norm(e0, (3, 0))
    assert z[0].tolist() == [0.0] * 3 and z[1].numel() == 0


def test_norm_of_the_segment_forms(EA, torch_cuda, block):
    for name in ("seg_ptr", "count"):
        f = block[name]
        got = EA.ops.gcn_norm(f["src"], (SIZE, ROWS), **f["kw"])
        want = EA.ops.gcn_norm((f["dst"], f["src"]), (SIZE, ROWS))
        assert same(got[0], want[0]) and same(got[1], want[1]) and float(want[0].sum()) > 0


def check_forward(torch, fused, composed, x, S):
    """fused(x, out_dtype) -> tensor; composed(x32) -> fp32 tensors to equal; the storage contract
    of the 16-bit ops (test_weighted_mp_gpu.check_forward)"""
    if S == torch.float32:
        got = fused(x, None)
        assert all(same(got, c) for c in composed(x))
        return
    want32 = fused(x.float(), None)
    assert all(same(want32, c) for c in composed(x.float()))
    assert same(fused(x, torch.float32), want32), "out fp32"
    gotS = fused(x, S)
    assert same(gotS, want32.to(S)), "out S"
    assert same(fused(x, None), gotS)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_forward_meets_contract_b(EA, torch_cuda, gen, block, which, d):
    torch = torch_cuda
    S = _dtypes(torch)[which]
    ops = EA.ops
    for unaligned in (False, True):
        x = draw(torch, gen, (ROWS, d), S, unaligned)
        for name, f in block.items():
            src, dst = f["src"], f["dst"]
            norm = ops.gcn_norm(edges_of(f), (SIZE, ROWS), **f["kw"])
            w = edge_weight(torch, norm, dst, src, SIZE)
            nd_np, ns_np = norm[0].cpu().numpy(), norm[1].cpu().numpy()
            dst_np, src_np = dst.cpu().numpy(), src.cpu().numpy()
            for op in OPS:
                def composed(t):
                    out = [ops.gather_scatter(op, t, src, dst, SIZE, edge_weight=w)]
                    if not unaligned:      # the restatement, once per (d, form, op)
                        r = ref.gcn_aggregate(op, t.cpu().numpy(), dst_np, src_np, SIZE, nd_np, ns_np)
                        out.append(torch.from_numpy(r).cuda())
                    return out
                check_forward(torch, lambda t, od: ops.gcn_aggregate(t, edges_of(f), (SIZE, ROWS), norm, op=op,
                                                                     out_dtype=od, **f["kw"]),
                              composed, x, S)
            # norm=None computes the same tables; two identical calls are bit-equal
            a = ops.gcn_aggregate(x, edges_of(f), (SIZE, ROWS), **f["kw"])
            assert same(a, ops.gcn_aggregate(x, edges_of(f), (SIZE, ROWS), norm, **f["kw"]))
            assert same(a, ops.gcn_aggregate(x, edges_of(f), (SIZE, ROWS), **f["kw"]))


def test_row_loop_strides_past_the_block_cap(EA, torch_cuda, gen):
    """32 769 destinations of one update each, d = 3: four rows a block, so the element form needs
    8 193 blocks and its cap of 8 192 makes the last row a second trip of the row loop"""
    torch = torch_cuda
    ops = EA.ops
    n, rows = 32769, 50
    x = draw(torch, gen, (rows, 3), torch.float32)
    src = torch.randint(0, rows, (n,), generator=gen, device="cuda", dtype=torch.int32)
    dst = torch.arange(n, device="cuda", dtype=torch.int32)
    norm = ops.gcn_norm(src, (n, rows), count=1)
    got = ops.gcn_aggregate(x, src, (n, rows), norm, count=1)
    w = edge_weight(torch, norm, dst, src, n)
    assert same(got, ops.gather_scatter("add", x, src, dst, n, edge_weight=w))
    assert same(got, w.reshape(-1, 1) * x[src.long()])        # one update: the message itself
    assert same(got, ops.gcn_aggregate(x, (dst, src), (n, rows), norm))


@pytest.mark.parametrize("op", OPS)
def test_empty_blocks_and_empty_tables(EA, torch_cuda, gen, op):
    """no edge, no source row or no destination: zeros (plus the root term), and gradients of zeros"""
    torch = torch_cuda
    ops = EA.ops
    d = 8
    none = torch.zeros((2, 0), dtype=torch.int32, device="cuda")
    some = torch.tensor([[0, 2, 1, 2], [1, 0, 3, 3]], dtype=torch.int32, device="cuda")
    for S in _dtypes(torch):
        # E == 0: keys, seg_ptr and no norm argument
        x = draw(torch, gen, (5, d), S).requires_grad_(True)
        root = draw(torch, gen, (3, d), S).requires_grad_(True)
        zero = torch.zeros((3, d), dtype=S, device="cuda")
        assert same(ops.gcn_aggregate(x, none, (3, 5), op=op), zero)
        sp = torch.zeros(4, dtype=torch.int64, device="cuda")
        assert same(ops.gcn_aggregate(x, none[1], (3, 5), op=op, seg_ptr=sp), zero)
        out = ops.gcn_aggregate(x, none, (3, 5), op=op, root=root, alpha=0.25)
        assert same(out, (root.float() * 0.25).to(S))
        out.backward(torch.ones_like(out))
        assert not bool(x.grad.any()) and same(root.grad, torch.full((3, d), 0.25, dtype=S, device="cuda"))
        # n_src == 0 with edges: every source index is out of range
        x0 = draw(torch, gen, (0, d), S).requires_grad_(True)
        out = ops.gcn_aggregate(x0, some, (3, 0), op=op)
        assert same(out, zero)
        out.sum().backward()
        assert x0.grad.shape == (0, d)
        # n_dst == 0 with edges: an empty output, and a gradient of zeros behind it
        x = draw(torch, gen, (5, d), S).requires_grad_(True)
        out = ops.gcn_aggregate(x, some, (0, 5), op=op)
        assert out.shape == (0, d)
        out.sum().backward()
        assert x.grad.shape == (5, d) and x.grad.dtype == S and not bool(x.grad.any())


def test_out_of_range_sources_contribute_nothing(EA, torch_cuda, gen, block):
    torch = torch_cuda
    ops = EA.ops
    f = block["unsorted"]
    src = f["src"].clone()
    src[::6] = ROWS
    src[1::11] = -1
    src[2::13] = 2 ** 31 - 1
    norm = ops.gcn_norm((f["dst"], src), (SIZE, ROWS))
    for d in (3, 64):
        for S in _dtypes(torch):
            x = draw(torch, gen, (ROWS, d), S)
            for op in OPS:
                got = ops.gcn_aggregate(x, (f["dst"], src), (SIZE, ROWS), norm, op=op, out_dtype=torch.float32)
                want = ref.gcn_aggregate(op, x.float().cpu().numpy(), f["dst"].cpu().numpy(), src.cpu().numpy(),
                                         SIZE, norm[0].cpu().numpy(), norm[1].cpu().numpy())
                assert same_np(torch, got, want), (d, S, op)


@pytest.mark.parametrize("d", [3, 64, 200])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_epilogue_meets_contract_c(EA, torch_cuda, gen, block, which, d):
    torch = torch_cuda
    S = _dtypes(torch)[which]
    ops = EA.ops
    alpha = 0.1
    for name in ("unsorted", "seg_ptr"):
        f = block[name]
        args = (edges_of(f), (SIZE, ROWS))
        for unaligned in (False, True):
            x = draw(torch, gen, (ROWS, d), S)
            for RS in {S, torch.float32}:
                root = draw(torch, gen, (SIZE, d), RS, unaligned)
                for op in OPS:
                    agg = ops.gcn_aggregate(x, *args, op=op, out_dtype=torch.float32, **f["kw"])
                    r32 = root.float()
                    for od in {S, torch.float32}:
                        got = ops.gcn_aggregate(x, *args, op=op, root=root, alpha=alpha, out_dtype=od, **f["kw"])
                        assert same(got, (agg * (1 - alpha) + r32 * alpha).to(od)), (name, RS, op, od)
                        got = ops.gcn_aggregate(x, *args, op=op, root=root, out_dtype=od, **f["kw"])
                        assert same(got, (agg + r32).to(od)), (name, RS, op, od)
                    got = ops.gcn_aggregate(x, *args, op=op, root=root, alpha=alpha, root_scale=0.5,
                                            out_dtype=torch.float32, **f["kw"])
                    assert same(got, agg * (1 - alpha) + r32 * 0.5)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["unsorted", "sorted", "seg_ptr", "count"])
def test_gradients_meet_contract_d(EA, torch_cuda, gen, block, name, op):
    torch = torch_cuda
    ops = EA.ops
    f = block[name]
    src, dst = f["src"], f["dst"]
    if name == "unsorted":
        # row ROWS - 1 is read only through destinations outside the block: its gradient is exactly 0
        src = torch.where(src == ROWS - 1, torch.zeros_like(src), src)
        src = torch.where((dst < 0) | (dst >= SIZE), torch.full_like(src, ROWS - 1), src)
    edges = src if f["kw"] else (dst, src)
    norm = ops.gcn_norm(edges, (SIZE, ROWS), **f["kw"])
    w = edge_weight(torch, norm, dst, src, SIZE)
    for d in (3, 64):
        for S in _dtypes(torch):
            for a, b, kw in ((1.0, 1.0, {}), (1 - 0.1, 0.1, dict(alpha=0.1)), (None, None, None)):
                x0 = draw(torch, gen, (ROWS, d), S)
                r0 = draw(torch, gen, (SIZE, d), S)
                g = draw(torch, gen, (SIZE, d), S)
                x, xc = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
                if kw is None:          # no root term
                    out = ops.gcn_aggregate(x, edges, (SIZE, ROWS), norm, op=op, **f["kw"])
                    comp = ops.gather_scatter(op, xc, src, dst, SIZE, edge_weight=w)
                    assert same(out, comp)
                    out.backward(g)
                    comp.backward(g)
                    assert same(x.grad, xc.grad), (d, S)
                else:
                    r, rc = r0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
                    out = ops.gcn_aggregate(x, edges, (SIZE, ROWS), norm, op=op, root=r, **kw, **f["kw"])
                    agg = ops.gather_scatter(op, xc, src, dst, SIZE, edge_weight=w, out_dtype=torch.float32)
                    comp = (agg * a + rc.float() * b).to(S)
                    assert same(out, comp)
                    out.backward(g)
                    comp.backward(g)
                    assert same(x.grad, xc.grad) and same(r.grad, rc.grad), (d, S, a)
                assert x.grad.dtype == S and float(x.grad.float().abs().sum()) > 0
                if name == "unsorted":
                    assert not bool(x.grad[ROWS - 1].any())


@pytest.mark.parametrize("op", OPS)
def test_against_float64_meets_contract_e(EA, torch_cuda, gen, block, op):
    torch = torch_cuda
    ops = EA.ops
    f = block["unsorted"]
    dst_np, src_np = f["dst"].cpu().numpy(), f["src"].cpu().numpy()
    for d in (3, 64):
        for S in _dtypes(torch):
            x = draw(torch, gen, (ROWS, d), S)
            want, scale, lens = ref.exact_f64(op, x.float().cpu().numpy(), dst_np, src_np, SIZE, ROWS)
            k = lens + 5 + (op == "mean")
            bound = (k * U / (1 - k * U))[:, None] * scale
            for od in {S, torch.float32}:
                got = ops.gcn_aggregate(x, (f["dst"], f["src"]), (SIZE, ROWS), op=op, out_dtype=od)
                b = bound
                if od != torch.float32:
                    mant, emin = (7, -126) if od == torch.bfloat16 else (10, -14)
                    exp = np.maximum(np.frexp(np.abs(want))[1].astype(np.float64) - 1, emin)
                    b = bound + 0.5 * 2.0 ** (exp - mant)
                err = np.abs(got.double().cpu().numpy() - want)
                assert np.all(err <= b), (d, S, od, float((err - b).max()))
            assert np.any(want != 0)


def test_errors(EA, torch_cuda, gen):
    torch = torch_cuda
    ops = EA.ops
    x = draw(torch, gen, (10, 12), torch.float32)
    dst = torch.tensor([0, 1, 1, 0, 1, 0], dtype=torch.int32, device="cuda")
    src = torch.tensor([3, 4, 9, 0, 2, 2], dtype=torch.int32, device="cuda")
    sp = torch.tensor([0, 2, 6], dtype=torch.int64, device="cuda")
    size = (2, 10)
    norm = ops.gcn_norm((dst, src), size)
    root = draw(torch, gen, (2, 12), torch.float32)
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x, (dst, src), size, norm, op="max")
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x, src, size, norm)                              # neither keys nor a segment form
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x, (dst, src), size, norm, count=3)              # both
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x, src, size, norm, seg_ptr=sp, count=3)
    with pytest.raises(ValueError):
        ops.gcn_norm(src, size)
    with pytest.raises(ValueError):
        ops.gcn_norm((dst, src), size, count=3)
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x, (dst.float(), src), size, norm)               # indices are integers, on both sides
    with pytest.raises(ValueError):
        ops.gcn_norm((dst, src.float()), size)
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x, src, size, norm, count=4)                     # E != n_dst * count
    with pytest.raises(ValueError):
        ops.gcn_norm(src, size, count=4)
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x, src, size, norm, seg_ptr=sp[:2])
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x, (dst, src), size, (norm[0], norm[1][:9]))      # wrong length
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x, (dst, src), size, (norm[1], norm[0]))
    with pytest.raises(TypeError):
        ops.gcn_aggregate(x, (dst, src), size, (norm[0].double(), norm[1]))
    with pytest.raises(TypeError):
        ops.gcn_aggregate(x, (dst, src), size, (norm[0], norm[1].half()))
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x, (dst, src), size, norm, root=root[:, :8])
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x, (dst, src), size, norm, root=x)               # [n_src, D], not [n_dst, D]
    with pytest.raises(TypeError):
        ops.gcn_aggregate(x, (dst, src), size, norm, root=root.half())     # neither fp32 nor x's dtype
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x, (dst, src), size, norm, alpha=0.1)            # alpha without root
    with pytest.raises(ValueError):
        ops.gcn_aggregate(x[:9], (dst, src), size, norm)
    with pytest.raises(TypeError):
        ops.gcn_aggregate(x.double(), (dst, src), size, norm)
    with pytest.raises(TypeError):
        ops.gcn_aggregate(x, (dst, src), size, norm, out_dtype=torch.float16)
    with pytest.raises(RuntimeError):
        ops.gcn_aggregate(x.cpu(), (dst, src), size, norm)
    bad = src.clone()
    bad[2] = 10
    with pytest.raises(IndexError):
        ops.gcn_aggregate(x, (dst, bad), size, norm, validate=True)
    ops.gcn_aggregate(x, (dst, src), size, norm, validate=True)
    # the raw C entries: the EINVAL ladder in its order, and nothing touched by a refused call
    L = EA._lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    out = torch.full((2, 12), 7.0, device="cuda")
    nd, ns = norm
    EINVAL = EA._lib.EINVAL

    def call(mode=0, x_=p(x), in_dt=0, rows=10, g=p(src), keys=p(dst), seg=None, count=0, e=6, d=12, n=2,
             nd_=p(nd), ns_=p(ns), root_=None, root_dt=0, out_=p(out), out_dt=0):
        return L.euler_gpu_gather_reduce_norm_t(None, mode, x_, in_dt, rows, g, keys, seg, count, e, d, n, nd_, ns_,
                                                root_, root_dt, 1.0, 1.0, out_, out_dt)

    def refused(text, **kw):
        assert call(**kw) == EINVAL, kw
        assert text in L.euler_gpu_last_error(), (kw, L.euler_gpu_last_error())

    refused(b"unknown dtype", in_dt=5, mode=1, e=-1)                       # dtype first
    refused(b"out_dtype", out_dt=1, mode=1)
    refused(b"root_dtype", root_=p(root), root_dt=2, mode=1)
    refused(b"max is not supported", mode=1, e=-1)                         # then mode
    refused(b"mode is", mode=3)
    refused(b"bad shape", e=-1, x_=None)                                   # then shape
    refused(b"bad shape", rows=-1)
    refused(b"exactly one", seg=p(sp))
    refused(b"exactly one", keys=None)
    refused(b"size * count", keys=None, count=4)
    refused(b"null buffer", x_=None, e=1 << 31)                            # null before e >= 2^31
    refused(b"null buffer", out_=None)
    refused(b"null buffer", ns_=None)
    refused(b"null buffer", e=0, keys=None, g=None, nd_=None)              # norm_dst is read per destination
    refused(b"null buffer", nd_=None, rows=0, x_=None, ns_=None)
    refused(b"mean needs", mode=2, keys=None, seg=p(sp), e=1 << 24)        # seg_ptr: no segment is longer than e
    refused(b"e >= 2^31", e=1 << 31, mode=2)                               # before the limit of a mean
    refused(b"mean needs", e=1 << 24, mode=2)
    refused(b"mean needs", mode=2, keys=None, count=1 << 24, e=2 << 24)
    refused(b"aligned", x_=C.c_void_p(x.data_ptr() + 2))
    refused(b"aligned", ns_=C.c_void_p(ns.data_ptr() + 2))
    assert call(n=0, x_=None) == 0 and call(d=0, out_=None) == 0           # nothing to do, nothing read
    nd_out, ns_out = torch.full((2,), 7.0, device="cuda"), torch.full((10,), 7.0, device="cuda")
    norm_call = lambda dk=p(dst), sk=p(src), e=6, a=2, b=10, o1=p(nd_out), o2=p(ns_out): \
        L.euler_gpu_gcn_norm(None, dk, sk, e, a, b, o1, o2)
    for kw, text in ((dict(e=-1), b"bad shape"), (dict(a=-2), b"bad shape"), (dict(dk=None), b"null buffer"),
                     (dict(o2=None), b"null buffer"), (dict(e=1 << 31), b"e >= 2^31"),
                     (dict(sk=C.c_void_p(src.data_ptr() + 2)), b"aligned")):
        assert norm_call(**kw) == EINVAL, kw
        assert text in L.euler_gpu_last_error(), kw
    assert norm_call(a=0, b=0, o1=None, o2=None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((nd_out == 7.0).all()) and bool((ns_out == 7.0).all())


def test_example_fused_equals_composed(EA, torch_cuda):
    torch = torch_cuda
    spec = importlib.util.spec_from_file_location(
        "gcn_norm_minibatch", os.path.join(ROOT, "examples", "python", "gcn_norm_minibatch.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    G = EA.Graph.load(os.path.join(ROOT, "tests", "golden", "fixture_dat"))
    max_id = int(G.id_range()[0])
    roots = torch.arange(1, min(max_id, 6) + 1, device="cuda", dtype=torch.int64)
    fused = ex.run(G, roots, 8)
    composed = ex.run(G, roots, 8, composed=True)
    assert fused.shape == (roots.numel(), 8) and float(fused.abs().sum()) > 0
    assert same(fused, composed)
