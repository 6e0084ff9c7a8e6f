"""The fused skip-gram loss head on the GPU (ops.skipgram_loss, euler_gpu_skipgram_loss[_grad]):
  A  forward bits == the numpy restatement tests/skipgram_ref.py (dtypes, d, unaligned views,
     the grid stride)
  B  per-occurrence gradient bits == the restatement; the tables' gradients == ops.scatter_add of
     those rows in occurrence order; sparse_grad; a shared table
  C  the loss and the table gradients within the derived bounds of the torch float64 composition
  D  both entries replay from a captured graph
  E  the rules of the C entries; empty shapes; guard words
  F  the example's steps on the fixture graph"""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_half_mp_gpu import DIMS
import skipgram_ref as ref

pytestmark = pytest.mark.gpu

NT, NC, B = 300, 280, 90
FIXTURE = os.path.join(ROOT, "tests", "golden", "fixture_dat")
PK = [(p, k) for p in (1, 2) for k in (0, 1, 5)]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def pairs(torch):
    f, b, h = torch.float32, torch.bfloat16, torch.float16
    return {"f32": (f, f), "bf16": (b, b), "f16": (h, h), "bf16-f32": (b, f), "f32-f16": (f, h)}


def draw(torch, gen, shape, S, unaligned=False):
    """values of dtype S in [-1, 1]; unaligned: a view that starts ONE ELEMENT into its storage"""
    x = ((torch.rand(shape, generator=gen, device="cuda") * 2) - 1).to(S)
    if unaligned:
        buf = torch.empty(x.numel() + 1, dtype=S, device="cuda")
        buf[1:] = x.reshape(-1)
        x = buf[1:].view(shape)
        assert x.data_ptr() % 16 == x.element_size() and x.is_contiguous()
    return x


class Batch(object):
    """B pair rows with P positives and K negatives over NT / NC rows: ids repeat inside the batch
    and some ids name no row (-1, rows + 3, 2^33 + 5), as test_triple_score_gpu.Batch"""

    def __init__(self, torch, p, k, seed=3, b=B, bad=True):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed + 10 * p + k)
        r = lambda hi, shape: torch.randint(0, hi, shape, generator=gen, device="cuda")      # noqa: E731
        self.p, self.k = p, k
        self.src, self.pos = r(NT, (b,)), r(NC, (b, p))
        self.neg = r(NC, (b, k)) if k else None
        self.src[5] = self.src[4]
        self.pos[6, 0] = self.pos[4, 0]
        if bad:
            self.src[10], self.src[13] = -1, (1 << 33) + 5
            self.pos[11, p - 1], self.pos[12, 0] = NC + 3, (1 << 33) + 5
        if k:
            self.neg[4, 0] = self.pos[4, 0]                     # the same row as positive and as negative: a tie
            self.neg[7, k - 1] = self.pos[6, 0]
            if bad:
                self.neg[15, 0], self.neg[16, k - 1], self.neg[10, 0] = -1, NC + 3, (1 << 33) + 5
        self.np = [None if t is None else t.cpu().numpy() for t in (self.src, self.pos, self.neg)]
        self.ids = (self.src, self.pos, self.neg)

    def context_keys(self):
        return np.concatenate([self.np[1].reshape(-1)] + ([self.np[2].reshape(-1)] if self.k else []))


@pytest.fixture(scope="module")
def batches(torch):
    return {pk: Batch(torch, *pk) for pk in PK}


def same(got, want):
    """two device tensors of one dtype and shape hold the same bits"""
    import torch
    as_int = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype in as_int:
        got, want = got.contiguous().view(as_int[got.dtype]), want.contiguous().view(as_int[want.dtype])
    return torch.equal(got, want)


def widened(t):
    return t.float().cpu().numpy()


def width(target, context):
    return ref.chunk_width(target.shape[1], target.data_ptr(), target.element_size(), context.data_ptr(),
                           context.element_size())


def np_same(got, want):
    got, want = got.cpu().numpy(), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


def configs(d, full):
    """(P, K): the full cross, or three per d, rotating"""
    if full:
        return PK
    i = DIMS.index(d)
    return [PK[(i + 2 * j) % 6] for j in range(3)]


def forward_raw(torch, target, context, bt):
    from euler_amd import ops
    return ops._skipgram_loss_raw(target, context, *bt.ids)


def check_forward(torch, target, context, bt, v):
    """the four outputs of the C entry and the three of the op == the restatement -> its outputs"""
    from euler_amd import ops
    want = ref.forward(widened(target), widened(context), *bt.np, v)
    loss, rank, logits, row_loss = forward_raw(torch, target, context, bt)
    tag = (bt.p, bt.k, v)
    assert np_same(logits, want[0]), tag + ("logits",)
    assert rank.dtype == torch.int32 and np.array_equal(rank.cpu().numpy(), want[1]), tag + ("rank",)
    assert np_same(row_loss, want[2]), tag + ("row_loss",)
    assert np_same(loss, np.array([want[3]], np.float32)), tag + ("loss",)
    out = ops.skipgram_loss(target, context, *bt.ids, return_logits=True)
    assert out[0].shape == () and same(out[0], loss.reshape(())) and same(out[1], rank) and same(out[2], logits)
    assert len(ops.skipgram_loss(target, context, *bt.ids)) == 2
    return want


# ---- A: forward bits -------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("S", ["f32", "bf16", "f16", "bf16-f32", "f32-f16"])
def test_forward_has_the_bits_of_the_restatement(torch, batches, S, d):
    ST, SC = pairs(torch)[S]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(100 + d)
    target, context = draw(torch, gen, (NT, d), ST), draw(torch, gen, (NC, d), SC)
    v = width(target, context)
    assert v == (8 if d % 8 == 0 else 4 if d % 4 == 0 else 1)
    for pk in configs(d, d in (1, 20, 520)):
        want = check_forward(torch, target, context, batches[pk], v)
        # the rank is the reference's double argsort on concat([neg, earlier positives | last positive])
        p = pk[0]
        others = np.concatenate([want[0][:, p:], want[0][:, :p - 1]], 1)
        assert np.array_equal(want[1], ref.mrr_score_ranks(want[0][:, p - 1:p], others))


@pytest.mark.parametrize("d", [8, 64, 520])
@pytest.mark.parametrize("S", ["f32", "bf16", "bf16-f32"])
def test_forward_and_gradient_on_unaligned_views(torch, batches, S, d):
    """tables that start one element into their storage: V = 1 (fp32: 4 bytes, 16-bit: 2 bytes in)"""
    from euler_amd import ops
    ST, SC = pairs(torch)[S]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(200 + d)
    target, context = draw(torch, gen, (NT, d), ST, unaligned=True), draw(torch, gen, (NC, d), SC, unaligned=True)
    assert width(target, context) == 1
    bt = batches[(2, 5)]
    want = check_forward(torch, target, context, bt, 1)
    g = torch.tensor([0.75], device="cuda")
    got = ops._skipgram_loss_grad_raw(target, context, *bt.ids, torch.from_numpy(want[0]).cuda(), g)
    want_g = ref.grad(widened(target), widened(context), *bt.np, want[0], 0.75)
    assert all(np_same(a, w) for a, w in zip(got, want_g))
    # one aligned table and one unaligned one: the rule looks at both
    target2 = draw(torch, gen, (NT, d), ST)
    assert width(target2, context) == 1
    check_forward(torch, target2, context, bt, 1)
    # the same table on both sides (LINE's first order)
    both = draw(torch, gen, (NT, d), ST)
    bt1 = Batch(torch, 1, 5, seed=77)
    check_forward(torch, both, both, bt1, width(both, both))


def test_grid_stride(torch):
    """d = 512 gives one pair row a wave and the launcher caps the grid at 32768 waves: with
    B = 33000 the rows from 32768 on are a wave's second task.  Rows are independent, so the
    restatement is taken for the first 64 and the last 300 only; the total is the restatement's
    reduction of the kernel's own row sums (129 rows a partial)."""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    d, b = 512, 33000
    sel = np.concatenate([np.arange(64), np.arange(b - 300, b)])
    pick = lambda ids: [None if t is None else t[sel] for t in ids]                      # noqa: E731
    target, context = draw(torch, gen, (NT, d), torch.float32), draw(torch, gen, (NC, d), torch.float32)
    bt = Batch(torch, 1, 1, seed=40, b=b)
    loss, rank, logits, row_loss = ops._skipgram_loss_raw(target, context, *bt.ids)
    want = ref.forward(widened(target), widened(context), *pick(bt.np), 8)
    assert logits.shape == (b, 2) and np_same(logits[sel], want[0]) and np_same(row_loss[sel], want[2])
    assert np.array_equal(rank[sel].cpu().numpy(), want[1])
    assert np_same(loss, np.array([ref.total(row_loss.cpu().numpy(), b, 1, 1)], np.float32))
    g = torch.tensor([-1.25], device="cuda")
    gs, gp, gn = ops._skipgram_loss_grad_raw(target, context, *bt.ids, logits, g)
    part = ref.grad(widened(target), widened(context), *pick(bt.np), want[0], -1.25, b_total=b)
    assert gs.shape == (b, d) and gp.shape == (b, 1, d) and gn.shape == (b, 1, d)
    assert np_same(gs[sel], part[0]) and np_same(gp[sel], part[1]) and np_same(gn[sel], part[2])


# ---- B: gradient bits ------------------------------------------------------------------------
def clean_keys(keys, rows):
    return np.where((keys >= 0) & (keys < rows), keys, -1).astype(np.int32)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("S", ["f32", "bf16", "f32-f16"])
def test_gradients_have_the_bits_of_the_restatement(torch, batches, S, d):
    """the kernel's rows == the restatement's; target.grad / context.grad == ops.scatter_add of the
    restatement's rows at src / [pos | neg] (ids that name no row: key -1), rounded once"""
    from euler_amd import ops
    ST, SC = pairs(torch)[S]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(300 + d)
    target, context = draw(torch, gen, (NT, d), ST), draw(torch, gen, (NC, d), SC)
    v = width(target, context)
    for j, pk in enumerate(configs(d, d in (3, 64, 520))):
        bt = batches[pk]
        g = float(np.float32(0.5 + j))
        logits = ref.forward(widened(target), widened(context), *bt.np, v)[0]
        got = ops._skipgram_loss_grad_raw(target, context, *bt.ids, torch.from_numpy(logits).cuda(),
                                          torch.tensor(g, device="cuda"))
        want = ref.grad(widened(target), widened(context), *bt.np, logits, g)
        for a, w, name in zip(got, want, ("src", "pos", "neg")):
            assert np_same(a, w), pk + (name,)
        if j:
            continue                                          # the autograd path: one (P, K) per d
        t, c = target.clone().requires_grad_(), context.clone().requires_grad_()
        loss, rank = ops.skipgram_loss(t, c, *bt.ids)
        assert not rank.requires_grad
        (loss * g).backward()
        want_t = ops.scatter_add(torch.from_numpy(want[0]).cuda(), torch.from_numpy(clean_keys(bt.np[0], NT)).cuda(),
                                 NT).to(ST)
        rows = np.concatenate([want[1].reshape(-1, d)] + ([want[2].reshape(-1, d)] if bt.k else []))
        want_c = ops.scatter_add(torch.from_numpy(rows).cuda(), torch.from_numpy(clean_keys(bt.context_keys(), NC)).cuda(),
                                 NC).to(SC)
        assert same(t.grad, want_t) and same(c.grad, want_c), pk
        assert t.grad.dtype == ST and c.grad.dtype == SC


@pytest.mark.parametrize("S", ["f32", "bf16"])
def test_sparse_grad_equals_the_dense_gradient_on_its_rows(torch, batches, S):
    from euler_amd import ops
    ST, SC = pairs(torch)[S]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    d = 20
    target, context = draw(torch, gen, (NT, d), ST), draw(torch, gen, (NC, d), SC)
    bt = batches[(2, 5)]
    grads = {}
    for sparse in (False, True):
        t, c = target.clone().requires_grad_(), context.clone().requires_grad_()
        loss, _ = ops.skipgram_loss(t, c, *bt.ids, sparse_grad=sparse)
        (loss * 3.0).backward()
        grads[sparse] = (t.grad, c.grad)
    for (dense, sp), keys, rows in zip(zip(*[grads[False], grads[True]]), (bt.np[0], bt.context_keys()), (NT, NC)):
        assert sp.is_sparse and sp.shape == dense.shape and sp.dtype == dense.dtype
        sp = sp.coalesce()
        idx = sp.indices()[0]
        looked_up = np.unique(keys[(keys >= 0) & (keys < rows)])
        assert np.array_equal(idx.cpu().numpy(), looked_up)               # absent elsewhere
        assert same(sp.values(), dense[idx])
        rest = torch.ones(rows, dtype=torch.bool, device="cuda")
        rest[idx] = False
        assert not bool(dense[rest].any())


@pytest.mark.parametrize("S", ["f32", "bf16"])
@pytest.mark.parametrize("sparse", [False, True])
def test_shared_table_gets_the_sum_of_both_parts(torch, S, sparse):
    """target and context the same tensor (LINE's first order): autograd adds the gradient of the
    target side and the gradient of the context side"""
    from euler_amd import ops
    ST = pairs(torch)[S][0]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(19)
    d = 64
    table = draw(torch, gen, (NC, d), ST)
    bt = Batch(torch, 1, 5, seed=50)
    bt.src.clamp_(max=NC - 1)
    ids = (bt.src, bt.pos, bt.neg)
    t = table.clone().requires_grad_()
    loss, rank, logits = ops.skipgram_loss(t, t, *ids, sparse_grad=sparse, return_logits=True)
    loss.backward()
    sep_t, sep_c = table.clone().requires_grad_(), table.clone().requires_grad_()
    loss2, rank2, logits2 = ops.skipgram_loss(sep_t, sep_c, *ids, return_logits=True)
    loss2.backward()
    assert same(loss, loss2) and same(rank, rank2) and same(logits, logits2)
    got = t.grad.to_dense() if sparse else t.grad
    assert t.grad.is_sparse == sparse and bool(sep_t.grad.any()) and bool(sep_c.grad.any())
    assert same(got, sep_t.grad + sep_c.grad)


def test_bad_ids_get_nothing_and_count_ln2(torch, batches):
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    d = 64
    target, context = draw(torch, gen, (NT, d), torch.float32), draw(torch, gen, (NC, d), torch.float32)
    bt = batches[(2, 5)]
    loss, rank, logits, row_loss = ops._skipgram_loss_raw(target, context, *bt.ids)
    gs, gp, gn = ops._skipgram_loss_grad_raw(target, context, *bt.ids, logits, torch.ones(1, device="cuda"))
    for rows, ids, n_rows in ((gs, bt.src, NT), (gp, bt.pos, NC), (gn, bt.neg, NC)):
        off = (ids < 0) | (ids >= n_rows)
        assert int(off.sum()) >= 2 and not bool(rows[off].any())
    live = (bt.src >= 0) & (bt.src < NT)
    assert bool(gs[live].any(-1).all())
    assert not bool(logits[~live].any())                                 # a bad src: every logit is 0
    ln2 = np.float32(0.6931472)
    seven = ln2
    for _ in range(6):
        seven = seven + ln2
    assert bool((row_loss[~live] == float(seven)).all())
    sp = torch.ones((4, 8), device="cuda", requires_grad=True)
    bad = torch.tensor([-1, 9, (1 << 33) + 5], device="cuda")
    loss, rank = ops.skipgram_loss(sp, sp, bad, bad.reshape(3, 1), bad.reshape(3, 1), sparse_grad=True)
    loss.backward()
    assert sp.grad.is_sparse and sp.grad.coalesce().indices().numel() == 0
    assert float(loss.detach()) == float(ref.total(np.full(3, ln2 + ln2, np.float32), 3, 1, 1))
    assert abs(float(loss.detach()) - np.log(2.0)) < 1e-6 and rank.tolist() == [1, 1, 1]          # 0 >= 0: the tie goes against the positive


# ---- C: the float64 composition --------------------------------------------------------------
def composition64(torch, target, context, src, pos, neg):
    """the reference's expressions in torch float64: the lookups (an id that names no row: zeros),
    PosNegLogits, sigmoid_cross_entropy_with_logits (labels 1: softplus(-x), labels 0:
    softplus(x)), the mean over the concatenation"""
    def look(table, ids):
        ok = (ids >= 0) & (ids < table.shape[0])
        return table[ids.clamp(0, table.shape[0] - 1)] * ok.unsqueeze(-1)

    softplus = lambda y: -torch.nn.functional.logsigmoid(-y)                             # noqa: E731
    t = look(target, src).unsqueeze(1)                                   # [B, 1, d]
    logits = torch.matmul(t, look(context, pos).transpose(1, 2))
    terms = [softplus(-logits).reshape(-1)]
    if neg is not None:
        terms.append(softplus(torch.matmul(t, look(context, neg).transpose(1, 2))).reshape(-1))
    return torch.cat(terms).mean()


# (unit roundoff, half the spacing of the subnormals) of the dtype a table gradient is rounded to
UNIT = {"f32": (0.0, 0.0), "bf16": (2.0 ** -8, 0.0), "f16": (2.0 ** -11, 2.0 ** -25)}


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("S", ["f32", "bf16", "f16"])
def test_within_the_derived_bounds_of_the_float64_composition(torch, batches, S, d, capsys):
    """the loss and the table gradients against the bounds derived in skipgram_ref.py, plus the
    one rounding of a 16-bit gradient; no margin.  16-bit tables are compared on their widened
    values."""
    from euler_amd import ops
    ST, SC = pairs(torch)[S]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(400 + d)
    target, context = draw(torch, gen, (NT, d), ST), draw(torch, gen, (NC, d), SC)
    worst_l = worst_g = 0.0
    for pk in configs(d, False)[:2]:
        bt = batches[pk]
        g = 1.5
        t, c = target.clone().requires_grad_(), context.clone().requires_grad_()
        loss, _ = ops.skipgram_loss(t, c, *bt.ids)
        (loss * g).backward()
        t64, c64 = target.double().requires_grad_(), context.double().requires_grad_()
        loss64 = composition64(torch, t64, c64, *bt.ids)
        (loss64 * g).backward()
        loss, loss64 = loss.detach(), loss64.detach()
        _, _, center, bound = ref.forward64(widened(target), widened(context), *bt.np)
        assert abs(float(loss64) - center) <= 1e-12 * (1 + abs(center)), pk          # the two float64 forms agree
        err = abs(float(loss.double()) - float(loss64))
        assert err <= bound, pk + (err / bound,)
        worst_l = max(worst_l, err / bound)
        (gs, bs), (gp, bp), (gn, bn) = ref.grad64(widened(target), widened(context), *bt.np, g)
        t_t, b_t = ref.table_grad64(gs, bs, bt.np[0], NT, *UNIT[S])
        t_c, b_c = ref.table_grad64(np.concatenate([gp.reshape(-1, d), gn.reshape(-1, d)]),
                                    np.concatenate([bp.reshape(-1, d), bn.reshape(-1, d)]), bt.context_keys(), NC,
                                    *UNIT[S])
        for got, want, center, bound in ((t.grad, t64.grad, t_t, b_t), (c.grad, c64.grad, t_c, b_c)):
            want = want.cpu().numpy()
            assert np.all(np.abs(want - center) <= 1e-9 * (1e-6 + np.abs(center))), pk  # the two float64 forms agree
            err = np.abs(got.double().cpu().numpy() - want)
            assert np.all(err <= bound), pk + (float(np.max(err / np.maximum(bound, 1e-300))),)
            worst_g = max(worst_g, float(np.max(err / np.maximum(bound, 1e-300))))
    with capsys.disabled():
        print("\n[skipgram_loss %s d=%d] worst error / bound: loss %.4f, table gradients %.4f" % (S, d, worst_l, worst_g))
    assert 0 < worst_l <= 1 and 0 < worst_g <= 1


# ---- D: captured graph -----------------------------------------------------------------------
def test_both_entries_replay_from_a_captured_graph(torch, batches):
    """one chain: the forward's two kernels, then the gradient kernel on the forward's logits"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    d = 128
    target, context = draw(torch, gen, (NT, d), torch.bfloat16), draw(torch, gen, (NC, d), torch.float32)
    bt = batches[(2, 5)]
    g = torch.tensor([0.5], device="cuda")
    want = ops._skipgram_loss_raw(target, context, *bt.ids)
    want_g = ops._skipgram_loss_grad_raw(target, context, *bt.ids, want[2], g)
    check_forward(torch, target, context, bt, width(target, context))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = ops._skipgram_loss_raw(target, context, *bt.ids)                                # (warm up)
        ops._skipgram_loss_grad_raw(target, context, *bt.ids, out[2], g)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = ops._skipgram_loss_raw(target, context, *bt.ids)
            out_g = ops._skipgram_loss_grad_raw(target, context, *bt.ids, out[2], g)
        for _ in range(2):
            for t in out + out_g:
                t.zero_()
            graph.replay()
            side.synchronize()
            assert all(same(a, b) for a, b in zip(out + out_g, want + want_g))
    torch.cuda.current_stream().wait_stream(side)


# ---- E: the C entries ------------------------------------------------------------------------
GUARD = -12345.0
PAD = 4                                                                  # guard words on each side (16 bytes)


class Call(object):
    """euler_gpu_skipgram_loss / _grad on small buffers with 4 guard words before and behind every output"""

    def __init__(self, torch):
        from euler_amd import _lib
        self.torch, self.lib = torch, _lib
        self.b, self.pp, self.k, self.d = 6, 2, 3, 8
        b, p, k, d = self.b, self.pp, self.k, self.d
        self.target = torch.ones((32, d), device="cuda")
        self.context = torch.ones((32, d), device="cuda")
        self.src = torch.arange(b, device="cuda")
        self.pos = torch.arange(b * p, device="cuda").reshape(b, p)
        self.neg = torch.arange(b * k, device="cuda").reshape(b, k)
        self.g = torch.ones(1, device="cuda")
        self.saved = torch.zeros(b * (p + k), device="cuda")
        self.sizes = dict(logits=b * (p + k), rank=b, row_loss=b, loss=1, g_src=b * d, g_pos=b * p * d, g_neg=b * k * d)
        self.out = {n: torch.full((s + 2 * PAD,), GUARD, device="cuda") for n, s in self.sizes.items()}

    def p(self, t, offset=0):
        return C.c_void_p(t.data_ptr() + 4 * offset)

    def head(self, a):
        return (a["target"], a["target_dt"], a["target_rows"], a["context"], a["context_dt"], a["context_rows"],
                a["src"], a["pos"], a["neg"], a["b"], a["p"], a["k"], a["d"])

    def base(self):
        base = dict(target=self.p(self.target), target_dt=self.lib.F32, target_rows=32, context=self.p(self.context),
                    context_dt=self.lib.F32, context_rows=32, src=self.p(self.src), pos=self.p(self.pos),
                    neg=self.p(self.neg), b=self.b, p=self.pp, k=self.k, d=self.d, saved=self.p(self.saved),
                    g=self.p(self.g))
        base.update({n: self.p(t, PAD) for n, t in self.out.items()})
        return base

    def forward(self, **kw):
        from euler_amd.ops import _stream
        a = dict(self.base(), **kw)
        rc = self.lib.lib().euler_gpu_skipgram_loss(_stream(), *self.head(a), a["logits"], a["rank"], a["row_loss"],
                                                    a["loss"])
        self.torch.cuda.synchronize()
        return rc

    def grad(self, **kw):
        from euler_amd.ops import _stream
        a = dict(self.base(), **kw)
        rc = self.lib.lib().euler_gpu_skipgram_loss_grad(_stream(), *self.head(a), a["saved"], a["g"], a["g_src"],
                                                         a["g_pos"], a["g_neg"])
        self.torch.cuda.synchronize()
        return rc

    def untouched(self, *names):
        return all(bool((self.out[n] == GUARD).all()) for n in (names or self.out))

    def written(self, name, size):
        """exactly [PAD, PAD + size) was written: the guard words before and behind are intact"""
        t = self.out[name]
        return not bool((t[PAD:PAD + size] == GUARD).any()) and bool((t[:PAD] == GUARD).all()) and \
            bool((t[PAD + size:] == GUARD).all())


def test_c_entry_error_rules(torch):
    c = Call(torch)
    EINVAL = c.lib.EINVAL
    for call in (c.forward, c.grad):
        assert call(target_dt=3) == EINVAL and call(context_dt=-1) == EINVAL
        assert call(k=-1) == EINVAL and call(b=-1) == EINVAL
        assert call(p=0) == EINVAL and call(d=0) == EINVAL and call(d=-1) == EINVAL
        assert call(neg=None) == EINVAL                                   # k > 0 without negatives
        assert call(target_rows=0) == EINVAL and call(context_rows=0) == EINVAL
        assert call(target_rows=1 << 31) == EINVAL and call(context_rows=1 << 31) == EINVAL
        assert call(b=1 << 29) == EINVAL                                  # b * (p + k) >= 2^31
        assert call(b=1 << 30, p=1, k=1) == EINVAL
        assert call(b=1 << 20, k=1 << 11) == EINVAL
        assert call(d=1 << 31) == EINVAL
        for name in ("target", "context", "src", "pos"):
            assert call(**{name: None}) == EINVAL, name
    for name in ("logits", "rank", "row_loss", "loss"):
        assert c.forward(**{name: None}) == EINVAL, name
    for name in ("saved", "g", "g_src", "g_pos", "g_neg"):
        assert c.grad(**{name: None}) == EINVAL, name
    assert c.untouched()


def test_c_entry_empty_shapes_and_guard_words(torch):
    c = Call(torch)
    OK = c.lib.OK
    # b == 0: the loss alone is written, +0; null buffers included
    assert c.forward(b=0) == OK and c.grad(b=0) == OK
    assert c.written("loss", 1) and float(c.out["loss"][PAD]) == 0.0 and not bool(torch.signbit(c.out["loss"][PAD]))
    assert c.untouched("logits", "rank", "row_loss", "g_src", "g_pos", "g_neg")
    c.out["loss"].fill_(GUARD)
    assert c.forward(b=0, target=None, src=None, pos=None, neg=None, logits=None, rank=None, row_loss=None) == OK
    assert c.grad(b=0, g_src=None, g=None, saved=None) == OK
    assert c.written("loss", 1) and float(c.out["loss"][PAD]) == 0.0
    # k == 0: the negative outputs stay untouched (and may be null)
    c = Call(torch)
    assert c.forward(k=0) == OK and c.grad(k=0) == OK
    assert c.untouched("g_neg")
    assert c.written("logits", c.b * c.pp) and c.written("rank", c.b) and c.written("row_loss", c.b)
    assert c.written("loss", 1) and c.written("g_src", c.b * c.d) and c.written("g_pos", c.b * c.pp * c.d)
    assert c.forward(k=0, neg=None) == OK and c.grad(k=0, neg=None, g_neg=None) == OK
    # the full call writes exactly [B, P + K] / [B] / [B] / [1] / [B, d] / [B, P, d] / [B, K, d]
    c = Call(torch)
    assert c.forward() == OK and c.grad() == OK
    for n, s in c.sizes.items():
        assert c.written(n, s), n
    assert c.out["rank"][PAD:PAD + c.b].view(torch.int32).tolist() == [c.pp - 1 + c.k] * c.b     # all rows equal: every tie counts


def test_python_argument_checks(torch):
    from euler_amd import ops
    t, c = torch.ones((4, 8), device="cuda"), torch.ones((5, 8), device="cuda")
    i = torch.zeros(3, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        ops.skipgram_loss(t, torch.ones((5, 4), device="cuda"), i, i.reshape(3, 1))
    with pytest.raises(ValueError):
        ops.skipgram_loss(t, c, i, i[:2].reshape(2, 1))
    with pytest.raises(ValueError):
        ops.skipgram_loss(t, c, i, i.reshape(3, 1), i[:2].reshape(2, 1))
    with pytest.raises(ValueError):
        ops.skipgram_loss(t, c, i, i[:0].reshape(3, 0))
    with pytest.raises(ValueError):
        ops.skipgram_loss(t[:, :0], c[:, :0], i, i.reshape(3, 1))
    with pytest.raises(TypeError):
        ops.skipgram_loss(t.double(), c, i, i.reshape(3, 1))
    with pytest.raises(RuntimeError):
        ops.skipgram_loss(t.cpu(), c, i, i.reshape(3, 1))
    with pytest.raises(ValueError):
        ops.rank_metric("hit5", i)
    loss, rank, logits = ops.skipgram_loss(t, c, i[:0], i[:0].reshape(0, 2), i[:0].reshape(0, 5), return_logits=True)
    assert loss.shape == () and float(loss) == 0 and rank.shape == (0,) and rank.dtype == torch.int32
    assert logits.shape == (0, 7)
    loss, rank = ops.skipgram_loss(t, c, i, i.reshape(3, 1), i[:0].reshape(3, 0))            # K = 0 as an empty tensor
    assert rank.tolist() == [0, 0, 0] and float(loss) > 0
    r = torch.tensor([0, 1, 3, 20], device="cuda", dtype=torch.int32)
    for name in ("mrr", "mr", "hit1", "hit3", "hit10"):
        got = ops.rank_metric(name, r)
        assert got.dtype == torch.float64 and abs(float(got) - ref.metric(name, [0, 1, 3, 20])) < 1e-15


# ---- F: the example's steps ------------------------------------------------------------------
@pytest.fixture(scope="module")
def example():
    spec = importlib.util.spec_from_file_location(
        "deepwalk_train", os.path.join(ROOT, "examples", "python", "deepwalk_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture()
def fixture_graph():
    """the fixture graph as the default graph of euler_ops for one test; the previous one comes back"""
    import euler_amd
    from euler_amd import euler_ops
    from euler_amd.euler_ops import base
    before = base._default
    G = euler_amd.Graph.load(FIXTURE)
    euler_ops.set_default_graph(G)
    yield G
    base._default = before


@pytest.mark.parametrize("order", [2, 1])
def test_example_steps_on_the_fixture_graph(torch, example, fixture_graph, order):
    """three SparseAdam steps of the example's loop on the fixture graph.  At every step the fused
    loss and the composed loss of the same tables agree within the bound of C on both sides of the
    float64 value (the composition's logits obey the same gamma(d) bound in any order, its
    softplus is the device's exp and log1p, its mean passes a term through fewer additions than
    the n of the bound), and rank_metric("mrr") equals the argsort restatement of mrr_score."""
    from euler_amd import ops
    G = fixture_graph
    G.set_seed(42)
    max_id = int(G.id_range()[0])
    target, context = example.make_tables(max_id, 32, order)
    assert (context is target) == (order == 1) and target.shape == (max_id + 2, 32)
    opt = torch.optim.SparseAdam([target] if order == 1 else [target, context], lr=0.01)
    for step in range(3):
        src, pos, negs = example.sample_step(16, max_id)
        assert bool(((src >= 0) & (src <= max_id + 1)).all()) and negs.shape[1] == 5
        before = target.detach().clone()
        with torch.no_grad():
            loss_c, rank_c, logits_c = example.loss_of(target, context, src, pos, negs, composed=True)
        loss, rank, logits = example.loss_of(target, context, src, pos, negs)
        fused, loss_c = float(loss.detach()), float(loss_c)
        ids = [t.cpu().numpy() for t in (src.reshape(-1), pos, negs)]
        _, _, loss64, bound = ref.forward64(widened(target.detach()), widened(context.detach()), *ids)
        print("\n[deepwalk example order %d step %d] fused %.9g composed %.9g float64 %.9g |diff| / (2 bound) = %.4f"
              % (order, step, fused, loss_c, loss64, abs(fused - loss_c) / (2 * bound)))
        assert abs(fused - loss64) <= bound
        assert abs(fused - loss_c) <= 2 * bound
        want_rank = ref.mrr_score_ranks(logits.cpu().numpy()[:, :1], logits.cpu().numpy()[:, 1:])
        assert np.array_equal(rank.cpu().numpy(), want_rank)
        assert abs(float(ops.rank_metric("mrr", rank)) - ref.metric("mrr", want_rank)) < 1e-15
        assert 0 < float(ops.rank_metric("mrr", rank)) <= 1
        opt.zero_grad()
        loss.backward()
        opt.step()
        moved = (target.detach() != before).any(1).cpu().numpy()
        want = np.zeros(max_id + 2, bool)
        want[ids[0]] = True
        if order == 1:
            want[ids[1].reshape(-1)] = True
            want[ids[2].reshape(-1)] = True
        assert np.array_equal(moved, want), (order, step)                # exactly the looked-up rows moved


@pytest.mark.parametrize("mode", [[], ["--composed"], ["--order", "1"]])
def test_example_runs(mode):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", "deepwalk_train.py"),
                        "--data", FIXTURE, "--batch", "16", "--steps", "3", "--dim", "32"] + mode,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("loss") == 3 and ("composed" in r.stdout) == ("--composed" in mode), r.stdout
