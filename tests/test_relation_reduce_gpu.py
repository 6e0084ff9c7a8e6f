"""The per-relation aggregation on the GPU (ops.relation_reduce / ops.relation_conv over
euler_gpu_relation_reduce):
  A  forward bits == the composition gather_scatter over the keys dst * R + type (-1: invalid)
  B  grad_params bits == torch autograd through that composition
  C  relation_conv against the reference's per-edge formulation in float64, derived bound
  D  the seg_ptr and count forms replay from a captured graph (no host wait)
  E  the EINVAL rules of the C entry, empty shapes, the grid stride
  F  a RelationDataFlow block and a sampled block with default_node fills, end to end
The small shapes - 300 table rows, 90 destinations, 10 draws (or ragged 0..70 updates) - take
every path: both lane shapes, the 8 / 4 / 1 batches, more than 64 updates, empty segments."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_half_mp_gpu import DIMS, bits, same

pytestmark = pytest.mark.gpu

ROWS, SIZE, COUNT = 300, 90, 10
OPS = ["add", "max", "mean", "mean_rel"]
AS_GS = {"add": "add", "max": "max", "mean_rel": "mean", "mean": "add"}
RELS = [1, 3, 8, 70]
FIXTURE = os.path.join(ROOT, "tests", "golden", "fixture_dat")


def draw(torch, gen, shape, S, unaligned=False):
    """values of dtype S in [-4, 4] (the pattern of test_half_mp_gpu.draw, for fp32 too); unaligned:
    a view that starts ONE ELEMENT into its storage - aligned to its type, not to 16 bytes"""
    x = ((torch.rand(shape, generator=gen, device="cuda") * 8) - 4).to(S)
    if unaligned:
        buf = torch.empty(x.numel() + 1, dtype=S, device="cuda")
        buf[1:] = x.reshape(-1)
        x = buf[1:].view(shape)
        assert x.data_ptr() % 16 == x.element_size() and x.is_contiguous()
    return x


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


class Form(object):
    """one way of naming the destinations, with its own updates: kw = the arguments of
    relation_reduce, dst = the destination of every update (int64, outside [0, size): none)"""

    def __init__(self, torch, gen, name, R):
        dev = "cuda"
        self.name, self.R = name, R
        if name == "count":
            self.e = SIZE * COUNT
            self.kw = {"count": COUNT}
            self.dst = torch.arange(SIZE, device=dev).repeat_interleave(COUNT)
        elif name == "seg_ptr":             # ragged 0..70, every ninth segment empty
            lens = torch.randint(1, 71, (SIZE,), generator=gen, device=dev)
            lens[::9] = 0
            lens[1], lens[2], lens[3] = 70, 1, 19
            sp = torch.zeros(SIZE + 1, dtype=torch.int64, device=dev)
            sp[1:] = lens.cumsum(0)
            self.e = int(sp[-1])
            self.kw = {"seg_ptr": sp}
            self.dst = torch.arange(SIZE, device=dev).repeat_interleave(lens)
        else:                               # unsorted keys, some < 0, some >= size
            self.e = SIZE * COUNT
            keys = torch.randint(-2, SIZE + 5, (self.e,), generator=gen, device=dev, dtype=torch.int32)
            self.kw = {"indices": keys}
            self.dst = keys.long()
        e = self.e
        t = torch.randint(-1, R + 1, (e,), generator=gen, device=dev, dtype=torch.int32)    # -1 and R: invalid
        if R >= 3:                          # relation 1 is absent from the whole input
            t = torch.where(t == 1, torch.full_like(t, R - 1), t)
        self.types = t
        self.valid = (self.dst >= 0) & (self.dst < SIZE) & (t >= 0) & (t < R)
        self.key = torch.where(self.valid, self.dst * R + t.long(), torch.full_like(self.dst, -1)).to(torch.int32)
        # rows 0 .. 289 are read by valid updates, rows 290 .. 299 by invalid ones only
        gi = torch.randint(0, ROWS - 10, (e,), generator=gen, device=dev, dtype=torch.int32)
        bad = torch.randint(ROWS - 10, ROWS, (e,), generator=gen, device=dev, dtype=torch.int32)
        self.gi = torch.where(self.valid, gi, bad)
        # int64 ids: some -1 and some past the table (both read the last row), some with high bits
        ids = self.gi.long()
        ids[5::17] = -1
        ids[7::19] = ROWS + 3
        ids[3::13] += 1 << 33
        self.ids = ids
        self.ids_rows = torch.clamp(ids & 0xFFFFFFFF, max=ROWS - 1).to(torch.int32)
        self.counts = torch.bincount(self.key[self.valid].long(), minlength=SIZE * R).view(SIZE, R).to(torch.int32)

    def composition(self, ops, torch, op, x, rows, out_dtype=None):
        """the same reduce spelled with the ops the parent commit has"""
        R = self.R
        if op != "mean":
            return ops.gather_scatter(AS_GS[op], x, rows, self.key, SIZE * R, out_dtype=out_dtype).view(SIZE, R, -1)
        s = ops.gather_scatter("add", x, rows, self.key, SIZE * R, out_dtype=torch.float32).view(SIZE, R, -1)
        out = s / (self.counts.sum(1) + 1e-7).view(SIZE, 1, 1)
        return out if out_dtype == torch.float32 else out.to(x.dtype)


@pytest.fixture(scope="module")
def forms(torch):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20)
    return {(name, R): Form(torch, gen, name, R) for R in RELS for name in ("count", "seg_ptr", "indices")}


def test_inputs_cover_the_cases(torch, forms):
    for (name, R), f in forms.items():
        assert int((f.types == -1).sum()) > 0 and int((f.types == R).sum()) > 0
        if R >= 3:
            assert int(f.counts[:, 1].sum()) == 0 and int(f.counts[:, 0].sum()) > 0
        if name == "indices":
            k = f.kw["indices"]
            assert int((k >= SIZE).sum()) > 0 and int((k < 0).sum()) > 0 and bool((k[1:] < k[:-1]).any())
        if name == "seg_ptr":
            lens = f.kw["seg_ptr"][1:] - f.kw["seg_ptr"][:-1]
            assert int(lens.max()) == 70 and int((lens == 0).sum()) >= 10
        assert int(f.counts.sum()) > 0 and f.e > ROWS


# ---- A: forward ------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RELS)
@pytest.mark.parametrize("d", DIMS)
def test_forward_fp32_has_the_bits_of_the_composition(torch, forms, R, d):
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 * R + d)
    for name in ("count", "seg_ptr", "indices"):
        f = forms[(name, R)]
        for unaligned in (False, True):
            full = draw(torch, gen, (f.e, d), torch.float32, unaligned)        # (e > ROWS: update p is row p)
            for op in OPS:
                for gather, rows in ((f.gi, f.gi), (f.ids, f.ids_rows), (None, torch.arange(f.e, device="cuda"))):
                    x = full if gather is None else full[:ROWS]
                    got, cnt = ops.relation_reduce(op, x, gather, f.types, R, SIZE, return_counts=True, **f.kw)
                    want = f.composition(ops, torch, op, x, rows)
                    assert same(got, want), (name, unaligned, op, gather is None or str(gather.dtype))
                    assert cnt.dtype == torch.int32 and torch.equal(cnt, f.counts)
        if R >= 3:      # empty buckets are written: 0, or -1e9 for max
            assert bool((got[:, 1] == 0).all())
            mx = ops.relation_reduce("max", full, f.gi, f.types, R, SIZE, **f.kw)
            assert bool((mx[:, 1] == -1e9).all())


@pytest.mark.parametrize("S", ["bfloat16", "float16"])
@pytest.mark.parametrize("R", [3, 70])
@pytest.mark.parametrize("d", DIMS)
def test_forward_16_bit_storage(torch, forms, S, R, d):
    """out_dtype=fp32: the bits of the fp32 op on x.float(); out_dtype=S: those bits after .to(S)"""
    from euler_amd import ops
    S = getattr(torch, S)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7000 + 10 * R + d)
    for name in ("count", "seg_ptr", "indices"):
        f = forms[(name, R)]
        for unaligned in (False, True):
            x = draw(torch, gen, (ROWS, d), S, unaligned)
            for op in OPS:
                for gather in (f.gi, f.ids):
                    want = ops.relation_reduce(op, x.float(), gather, f.types, R, SIZE, **f.kw)
                    wide, cnt = ops.relation_reduce(op, x, gather, f.types, R, SIZE, out_dtype=torch.float32,
                                                    return_counts=True, **f.kw)
                    assert same(wide, want), (name, unaligned, op)
                    assert same(ops.relation_reduce(op, x, gather, f.types, R, SIZE, **f.kw), want.to(S))
                    assert torch.equal(cnt, f.counts)


# ---- B: gradient -----------------------------------------------------------------------------
@pytest.mark.parametrize("S", ["float32", "bfloat16"])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("d", [8, 20])
def test_grad_params_has_the_bits_of_autograd_through_the_composition(torch, forms, S, op, d):
    from euler_amd import ops
    S = getattr(torch, S)
    R = 3
    gen = torch.Generator(device="cuda")
    gen.manual_seed(300 + d)
    for name in ("count", "seg_ptr", "indices"):
        f = forms[(name, R)]
        x = draw(torch, gen, (ROWS, d), S)
        g = draw(torch, gen, (SIZE, R, d), S)
        for gather, rows in ((f.gi, f.gi), (f.ids, f.ids_rows)):
            a = x.clone().requires_grad_(True)
            ops.relation_reduce(op, a, gather, f.types, R, SIZE, **f.kw).backward(g)
            b = x.clone().requires_grad_(True)
            f.composition(ops, torch, op, b, rows).backward(g)
            assert same(a.grad, b.grad), (name, str(gather.dtype))
            assert int(a.grad.abs().sum() > 0)
            if gather is f.gi:          # rows read by invalid updates only: exactly 0
                assert bool((bits(a.grad[ROWS - 10:]) == 0).all())
    # no gather: update p is row p
    f = forms[("count", R)]
    x = draw(torch, gen, (f.e, d), S)
    g = draw(torch, gen, (SIZE, R, d), S)
    a = x.clone().requires_grad_(True)
    ops.relation_reduce(op, a, None, f.types, R, SIZE, **f.kw).backward(g)
    b = x.clone().requires_grad_(True)
    f.composition(ops, torch, op, b, torch.arange(f.e, device="cuda")).backward(g)
    assert same(a.grad, b.grad)
    assert bool((bits(a.grad[~f.valid]) == 0).all())


# ---- C: relation_conv against the reference's formulation -------------------------------------
def reference_conv(torch, x, w, rows, types, dst, size):
    """relation_conv.py:63-70 then scatter_mean (mp_ops.py:65-69): one matrix per edge"""
    msg = torch.bmm(w[types], x[rows].unsqueeze(-1)).squeeze(-1)                 # [E, dim]
    s = torch.zeros((size, w.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, dst, msg)
    deg = torch.zeros(size, dtype=x.dtype, device=x.device).index_add_(0, dst, torch.ones_like(dst, dtype=x.dtype))
    return s / (deg + 1e-7).unsqueeze(1)


def gamma(n):
    u = 2.0 ** -24
    return n * u / (1 - n * u)


def check_conv(torch, x, w, gather, types, dst, size, l_max, m_max, **kw):
    """Bounds (derived; gamma_n = n u / (1 - n u), u = 2^-24, the bound of any order of n correctly
    rounded fp32 operations on a sum of products, applied to the sum of the terms' magnitudes):
      out      n = F + L_max + 2: at most L_max adds of a bucket, the denominator's add and the
               divide, then the dot product over F columns (issue text);
      grad_x   n = dim + M_max + 2: the dot product over dim, the denominator and the divide, then
               at most M_max adds into a row of x read by M_max updates;
      grad_w   n = size + L_max + 2: a bucket's adds, denominator and divide, then the sum over the
               destinations."""
    from euler_amd import ops
    R, dim, F = w.shape
    rows = gather.long()
    g = ((torch.rand((size, dim), device="cuda") * 2) - 1)
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        a, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        out = ops.relation_conv(a, wa, gather, types, size, aggr="mean", **kw)
        out.backward(g)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    want = reference_conv(torch, x64, w64, rows, types.long(), dst, size)
    want.backward(g.double())
    xa, wa_ = x.double().abs().requires_grad_(True), w.double().abs().requires_grad_(True)
    mag = reference_conv(torch, xa, wa_, rows, types.long(), dst, size)          # sum |W x| / deg
    mag.backward(g.double().abs())
    for what, got, ref, m, n in (("out", out, want, mag, F + l_max + 2),
                                 ("grad_x", a.grad, x64.grad, xa.grad, dim + m_max + 2),
                                 ("grad_w", wa.grad, w64.grad, wa_.grad, size + l_max + 2)):
        err = (got.detach().double() - ref.detach()).abs()
        bound = gamma(n) * m.detach()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print("relation_conv %s: max error / bound = %.3f (n = %d)" % (what, worst, n))
        assert bool((err <= bound).all()), (what, worst)


def test_relation_conv_against_the_per_edge_formulation(torch):
    R, F, dim = 3, 20, 8
    gen = torch.Generator(device="cuda")
    gen.manual_seed(77)
    x = draw(torch, gen, (ROWS, F), torch.float32)
    w = draw(torch, gen, (R, dim, F), torch.float32)
    # a sampled block: count draws a destination
    e = SIZE * COUNT
    gi = torch.randint(0, ROWS, (e,), generator=gen, device="cuda", dtype=torch.int32)
    t = torch.randint(0, R, (e,), generator=gen, device="cuda", dtype=torch.int32)
    dst = torch.arange(SIZE, device="cuda").repeat_interleave(COUNT)
    m_max = int(torch.bincount(gi.long()).max())
    check_conv(torch, x, w, gi, t, dst, SIZE, COUNT, m_max, count=COUNT)
    # a full-neighbour block: ragged segments 0 .. 70
    lens = torch.randint(0, 71, (SIZE,), generator=gen, device="cuda")
    lens[0], lens[1] = 70, 0
    sp = torch.zeros(SIZE + 1, dtype=torch.int64, device="cuda")
    sp[1:] = lens.cumsum(0)
    e = int(sp[-1])
    gi = torch.randint(0, ROWS, (e,), generator=gen, device="cuda", dtype=torch.int32)
    t = torch.randint(0, R, (e,), generator=gen, device="cuda", dtype=torch.int32)
    dst = torch.arange(SIZE, device="cuda").repeat_interleave(lens)
    m_max = int(torch.bincount(gi.long()).max())
    check_conv(torch, x, w, gi, t, dst, SIZE, 70, m_max, seg_ptr=sp)
    # unsorted keys name the same block
    p = torch.randperm(e, generator=gen, device="cuda")
    check_conv(torch, x, w, gi[p], t[p], dst[p], SIZE, 70, m_max, indices=dst[p].to(torch.int32))


# ---- D: no host wait -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seg_ptr", "count"])
def test_no_host_wait(torch, forms, name):
    """the call is captured into a graph on a side stream and replays to the same bits"""
    from euler_amd import ops
    f = forms[(name, 8)]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    x = draw(torch, gen, (ROWS, 64), torch.float32)
    want = f.composition(ops, torch, "mean", x, f.ids_rows)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.relation_reduce("mean", x, f.ids, f.types, 8, SIZE, return_counts=True, **f.kw)      # (warm up)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out, cnt = ops.relation_reduce("mean", x, f.ids, f.types, 8, SIZE, return_counts=True, **f.kw)
        for _ in range(2):
            out.zero_()
            cnt.zero_()
            g.replay()
            side.synchronize()
            assert same(out, want) and torch.equal(cnt, f.counts)
    torch.cuda.current_stream().wait_stream(side)


# ---- E: edge cases ---------------------------------------------------------------------------
def test_c_abi_error_rules(torch):
    from euler_amd import _lib
    from euler_amd.ops import _stream
    L = _lib.lib()
    size, R, d, count = 6, 3, 8, 4
    e = size * count
    x = torch.ones((32, d), device="cuda")
    gi = torch.zeros(e, dtype=torch.int32, device="cuda")
    t = torch.zeros(e, dtype=torch.int32, device="cuda")
    keys = torch.zeros(e, dtype=torch.int32, device="cuda")
    sp = torch.arange(size + 1, dtype=torch.int64, device="cuda") * count
    guard = -12345.0
    out = torch.full((size, R, d), guard, device="cuda")
    p = lambda v: C.c_void_p(v.data_ptr())                     # noqa: E731
    base = dict(mode=0, params=p(x), in_dt=_lib.F32, rows=32, gather=p(gi), is_ids=0, types=p(t), R=R,
                indices=None, seg_ptr=None, count=count, e=e, d=d, size=size, out=p(out), out_dt=_lib.F32,
                counts=None)

    def call(**kw):
        a = dict(base, **kw)
        rc = L.euler_gpu_relation_reduce(_stream(), a["mode"], a["params"], a["in_dt"], a["rows"], a["gather"],
                                         a["is_ids"], a["types"], a["R"], a["indices"], a["seg_ptr"], a["count"],
                                         a["e"], a["d"], a["size"], a["out"], a["out_dt"], a["counts"])
        torch.cuda.synchronize()
        return rc

    EINVAL = _lib.EINVAL
    assert call(mode=-1) == EINVAL and call(mode=4) == EINVAL
    assert call(R=0) == EINVAL
    assert call(size=1 << 30, R=2, count=0, seg_ptr=p(sp), e=e) == EINVAL          # size * R >= 2^31
    assert call(e=1 << 31, count=0, indices=p(keys)) == EINVAL
    assert call(mode=2, e=1 << 24, count=0, indices=p(keys)) == EINVAL            # a mean: e >= 2^24
    assert call(mode=3, e=1 << 24, count=0, seg_ptr=p(sp)) == EINVAL
    assert call(mode=2, count=1 << 24, size=1, e=1 << 24) == EINVAL
    assert call(count=0) == EINVAL                                               # no segment form
    assert call(indices=p(keys)) == EINVAL and call(seg_ptr=p(sp)) == EINVAL      # two forms
    assert call(indices=p(keys), seg_ptr=p(sp), count=0) == EINVAL
    assert call(e=e + 1) == EINVAL                                               # e != size * count
    assert call(params=None) == EINVAL and call(types=None) == EINVAL and call(out=None) == EINVAL
    assert call(in_dt=3) == EINVAL and call(in_dt=-1) == EINVAL and call(out_dt=7) == EINVAL
    assert call(in_dt=_lib.BF16, out_dt=_lib.F16) == EINVAL                      # neither fp32 nor in_dtype
    assert call(in_dt=_lib.F32, out_dt=_lib.BF16) == EINVAL
    assert call(gather=None, rows=e - 1) == EINVAL                               # update p is row p: too few rows
    assert bool((out == guard).all())                                            # nothing was written
    assert call(size=0, count=0, seg_ptr=p(sp), e=0) == 0 and call(d=0) == 0
    assert bool((out == guard).all())
    assert call() == 0 and bool((out[:, 0] == count).all()) and bool((out[:, 1:] == 0).all())


def test_empty_shapes(torch):
    from euler_amd import ops
    x = torch.ones((4, 8), device="cuda")
    none32 = torch.zeros(0, dtype=torch.int32, device="cuda")
    out, cnt = ops.relation_reduce("add", x, none32, none32, 3, 0, indices=none32, return_counts=True)
    assert out.shape == (0, 3, 8) and cnt.shape == (0, 3)
    # e == 0 with size > 0 writes the empty values
    for op, value in (("add", 0.0), ("max", -1e9), ("mean", 0.0), ("mean_rel", 0.0)):
        for kw in ({"indices": none32}, {"seg_ptr": torch.zeros(6, dtype=torch.int64, device="cuda")}):
            out, cnt = ops.relation_reduce(op, x, none32, none32, 3, 5, return_counts=True, **kw)
            assert out.shape == (5, 3, 8) and bool((out == value).all()) and not bool(cnt.any())
    a = x.clone().requires_grad_(True)
    ops.relation_reduce("mean", a, none32, none32, 3, 5, indices=none32).sum().backward()
    assert not bool(a.grad.any())


def test_grid_stride(torch):
    """40 000 destinations: four a block on the one-column-per-lane path (an unaligned table) is
    more blocks than the cap of 8192, so the grid strides"""
    from euler_amd import ops
    size, d, count, R = 40_000, 8, 2, 2
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    e = size * count
    gi = torch.randint(0, ROWS, (e,), generator=gen, device="cuda", dtype=torch.int32)
    t = torch.randint(-1, R, (e,), generator=gen, device="cuda", dtype=torch.int32)
    dst = torch.arange(size, device="cuda").repeat_interleave(count)
    key = torch.where(t >= 0, dst * R + t, torch.full_like(dst, -1)).to(torch.int32)
    for unaligned in (False, True):
        x = draw(torch, gen, (ROWS, d), torch.float32, unaligned)
        got, cnt = ops.relation_reduce("mean_rel", x, gi, t, R, size, count=count, return_counts=True)
        assert same(got, ops.gather_scatter("mean", x, gi, key, size * R).view(size, R, d))
        assert torch.equal(cnt.view(-1).long(), torch.bincount(key[key >= 0].long(), minlength=size * R))


def test_python_argument_checks(torch):
    from euler_amd import ops
    x = torch.ones((4, 8), device="cuda")
    i = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.relation_reduce("sum", x, i, i, 2, 2, count=2)
    with pytest.raises(ValueError):
        ops.relation_reduce("add", x, i, i, 2, 2)
    with pytest.raises(ValueError):
        ops.relation_reduce("add", x, i, i, 2, 2, count=2, indices=i)
    with pytest.raises(ValueError):
        ops.relation_reduce("add", x, i, i, 2, 3, count=2)
    with pytest.raises(TypeError):
        ops.relation_reduce("add", x.double(), i, i, 2, 2, count=2)
    with pytest.raises(RuntimeError):
        ops.relation_reduce("add", x.cpu(), i.cpu(), i.cpu(), 2, 2, count=2)
    with pytest.raises(ValueError):
        ops.relation_conv(x, torch.ones((2, 3, 8), device="cuda"), i, i, 2, count=2, aggr="max")


# ---- F: end to end ---------------------------------------------------------------------------
def test_relation_dataflow_block_through_relation_conv(torch):
    import euler_amd
    from euler_amd.dataflow import RelationDataFlow
    G = euler_amd.Graph.load(FIXTURE)
    roots = torch.tensor([1, 2, 3, 4, 5, 6, 2], device="cuda")
    blk = RelationDataFlow(G, [[0, 1]])(roots).blocks[0]
    dst, src, types = blk.edge_index[0], blk.edge_index[1], blk.e_id
    e = int(types.numel())
    assert e > 0 and set(types.cpu().tolist()) == {0, 1}
    R, F, dim = 3, 20, 8                                 # relation 2 has no edge
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4)
    x = draw(torch, gen, (int(blk.n_id.numel()), F), torch.float32)
    w = draw(torch, gen, (R, dim, F), torch.float32)
    size = int(blk.size[0])
    l_max = int(torch.bincount(dst.long(), minlength=size).max())
    m_max = int(torch.bincount(src.long()).max())
    check_conv(torch, x, w, src.to(torch.int32), types, dst.long(), size, l_max, m_max,
               indices=dst.to(torch.int32))


def test_sampled_block_with_default_fills(torch):
    """the fills of sample_neighbor carry type -1 and drop out without a mask: the same bits as
    the call on the block with the filled entries removed by hand"""
    import euler_amd
    from euler_amd import ops
    G = euler_amd.Graph.load(FIXTURE)
    G.set_seed(3)
    nodes = torch.tensor([1, 2, 99, 3, 4, 5, 6, 1234], device="cuda")        # 99, 1234: not in the graph
    count, default = 5, 7
    ids, _w, types = G.sample_neighbor(nodes, [0, 1], count, default_node=default, call_id=1)
    ids, types = ids.reshape(-1), types.reshape(-1)
    filled = ids == default
    assert int(filled.sum()) >= 2 * count and bool((types[filled] == -1).all()) and bool((types[~filled] >= 0).all())
    R, F, dim = 2, 20, 8
    gen = torch.Generator(device="cuda")
    gen.manual_seed(6)
    x = draw(torch, gen, (default + 1, F), torch.float32)                    # row = node id
    w = draw(torch, gen, (R, dim, F), torch.float32)
    n = int(nodes.numel())
    keep = ~filled
    lens = keep.view(n, count).sum(1)
    sp = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    sp[1:] = lens.cumsum(0)
    for aggr in ("mean", "mean_rel", "add"):
        got = ops.relation_conv(x, w, ids, types, n, count=count, aggr=aggr)
        want = ops.relation_conv(x, w, ids[keep], types[keep], n, seg_ptr=sp, aggr=aggr)
        assert same(got, want), aggr
    assert not bool(got[2].any()) and not bool(got[7].any()) and bool(got[0].any())


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", "rgcn_minibatch.py")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    losses = [float(line.split("loss")[1].split()[0]) for line in r.stdout.splitlines() if "loss" in line]
    assert len(losses) == 2 and all(np.isfinite(losses)), r.stdout
