"""The fused triple scoring on the GPU (ops.triple_score, euler_gpu_triple_score[_grad]):
  A  forward bits == the numpy restatement tests/triple_score_ref.py (dtypes, d, unaligned views,
     the grid stride)
  B  per-occurrence gradient bits == the restatement; the tables' gradients == ops.scatter_add of
     those rows in occurrence order; sparse_grad; repeated and out-of-range ids
  C  forward and table gradients within the derived bounds of the torch float64 composition
  D  both entries replay from a captured graph
  E  the rules of the C entries; empty shapes; guard words
  F  the example's step on the fixture graph"""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_half_mp_gpu import DIMS, same
import triple_score_ref as ref

pytestmark = pytest.mark.gpu

ENT, REL, B = 300, 7, 90
KINDS, CORRUPTS = ("trans_l1", "trans_l2", "distmult"), ("front", "tail", "both")
FIXTURE = os.path.join(ROOT, "tests", "golden", "fixture_dat")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def pairs(torch):
    f, b, h = torch.float32, torch.bfloat16, torch.float16
    return {"f32": (f, f), "bf16": (b, b), "f16": (h, h), "bf16-f32": (b, f), "f32-f16": (f, h)}


def draw(torch, gen, shape, S, unaligned=False):
    """values of dtype S in [-4, 4]; unaligned: a view that starts ONE ELEMENT into its storage"""
    x = ((torch.rand(shape, generator=gen, device="cuda") * 8) - 4).to(S)
    if unaligned:
        buf = torch.empty(x.numel() + 1, dtype=S, device="cuda")
        buf[1:] = x.reshape(-1)
        x = buf[1:].view(shape)
        assert x.data_ptr() % 16 == x.element_size() and x.is_contiguous()
    return x


class Batch(object):
    """B triples with K negatives over ENT / REL rows: ids repeat inside the batch, a negative
    equals its src, and some ids name no row (-1, rows + 3, 2^33 + 5)"""

    def __init__(self, torch, k, seed=3, b=B, bad=True):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed + k)
        r = lambda hi, shape: torch.randint(0, hi, shape, generator=gen, device="cuda")      # noqa: E731
        self.k = k
        self.src, self.dst, self.rel_id = r(ENT, (b,)), r(ENT, (b,)), r(REL, (b,))
        self.neg = r(ENT, (b, k)) if k else None
        self.src[5] = self.src[4]
        self.dst[6] = self.src[4]
        if bad:
            self.src[10], self.dst[11], self.rel_id[12] = -1, ENT + 3, (1 << 33) + 5
            self.src[13], self.rel_id[14] = (1 << 33) + 5, -1
        if k:
            self.neg[4, 0] = self.src[4]
            self.neg[7, k - 1] = self.dst[6]
            if bad:
                self.neg[15, 0], self.neg[16, k - 1] = -1, ENT + 3
        self.np = [None if t is None else t.cpu().numpy() for t in (self.src, self.rel_id, self.dst, self.neg)]
        self.ids = (self.src, self.rel_id, self.dst, self.neg)

    def ent_keys(self):
        return np.concatenate([self.np[0], self.np[2]] + ([self.np[3].reshape(-1)] if self.k else []))


@pytest.fixture(scope="module")
def batches(torch):
    return {k: Batch(torch, k) for k in (0, 1, 5)}


def widened(t):
    return t.float().cpu().numpy()


def width(ent, rel):
    return ref.chunk_width(ent.shape[1], ent.data_ptr(), ent.element_size(), rel.data_ptr(), rel.element_size())


def np_same(got, want):
    got = got.cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


def configs(d, full):
    """(kind, corrupt, normalize, K): the full cross, or one kind per d with the rest rotating"""
    if full:
        return [(kind, c, nz, k) for kind in KINDS for nz in (True, False) for k in (0, 1, 5)
                for c in (CORRUPTS if k else ("both",))]
    i = DIMS.index(d)
    return [(KINDS[i % 3], CORRUPTS[(i + j) % 3], j % 2 == 0, k) for j, k in enumerate((0, 1, 5))]


# ---- A: forward bits -------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("S", ["f32", "bf16", "f16", "bf16-f32", "f32-f16"])
def test_forward_has_the_bits_of_the_restatement(torch, batches, S, d):
    from euler_amd import ops
    SE, SR = pairs(torch)[S]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(100 + d)
    ent, rel = draw(torch, gen, (ENT, d), SE), draw(torch, gen, (REL, d), SR)
    v = width(ent, rel)
    assert v == (8 if d % 8 == 0 else 4 if d % 4 == 0 else 1)
    for kind, corrupt, normalize, k in configs(d, d in (1, 20, 520)):
        bt = batches[k]
        got = ops.triple_score(ent, rel, *bt.ids, kind=kind, corrupt=corrupt, normalize=normalize)
        want_pos, want_neg = ref.forward(widened(ent), widened(rel), *bt.np, kind, corrupt, normalize, v)
        tag = (kind, corrupt, normalize, k)
        if k == 0:
            assert torch.is_tensor(got) and np_same(got, want_pos), tag
        else:
            assert np_same(got[0], want_pos) and np_same(got[1], want_neg), tag
            assert got[1].shape == (B, 2 * k if corrupt == "both" else k)


@pytest.mark.parametrize("d", [8, 64, 520])
@pytest.mark.parametrize("S", ["f32", "bf16", "bf16-f32"])
def test_forward_and_gradient_on_unaligned_views(torch, batches, S, d):
    """tables that start one element into their storage: V = 1 (fp32: 4 bytes, 16-bit: 2 bytes in)"""
    from euler_amd import ops
    SE, SR = pairs(torch)[S]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(200 + d)
    ent, rel = draw(torch, gen, (ENT, d), SE, unaligned=True), draw(torch, gen, (REL, d), SR, unaligned=True)
    v = width(ent, rel)
    assert v == 1
    bt = batches[5]
    for kind in KINDS:
        pos, neg = ops.triple_score(ent, rel, *bt.ids, kind=kind)
        want = ref.forward(widened(ent), widened(rel), *bt.np, kind, "both", True, v)
        assert np_same(pos, want[0]) and np_same(neg, want[1]), kind
        g_pos, g_neg = draw(torch, gen, (B,), torch.float32), draw(torch, gen, (B, 10), torch.float32)
        got = ops._triple_score_grad_raw(ent, rel, *bt.ids, kind, "both", True, g_pos, g_neg)
        want = ref.grad(widened(ent), widened(rel), *bt.np, kind, "both", True, v, widened(g_pos), widened(g_neg))
        assert all(np_same(g, w) for g, w in zip(got, want)), kind
    # one aligned table and one unaligned one: the rule looks at both
    ent2 = draw(torch, gen, (ENT, d), SE)
    assert width(ent2, rel) == 1
    pos, neg = ops.triple_score(ent2, rel, *bt.ids, kind="distmult")
    want = ref.forward(widened(ent2), widened(rel), *bt.np, "distmult", "both", True, 1)
    assert np_same(pos, want[0]) and np_same(neg, want[1])


def test_grid_stride(torch):
    """d = 512 gives one triple a wave and the launcher caps the grid at 32768 waves: with B = 33000
    the triples from 32768 on are a wave's second task.  Triples are independent, so the
    restatement is taken for the first 64 and the last 300 only."""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    d, b = 512, 33000
    sel = np.concatenate([np.arange(64), np.arange(b - 300, b)])
    pick = lambda ids: [None if t is None else t[sel] for t in ids]                      # noqa: E731
    ent, rel = draw(torch, gen, (ENT, d), torch.float32), draw(torch, gen, (REL, d), torch.float32)
    bt = Batch(torch, 1, seed=40, b=b)
    pos, neg = ops.triple_score(ent, rel, *bt.ids, kind="distmult", corrupt="tail")
    want = ref.forward(widened(ent), widened(rel), *pick(bt.np), "distmult", "tail", True, 8)
    assert pos.shape == (b,) and np_same(pos[sel], want[0]) and np_same(neg[sel], want[1])
    b0 = Batch(torch, 0, seed=41, b=b)
    g_pos = draw(torch, gen, (b,), torch.float32)
    got = ops._triple_score_grad_raw(ent, rel, *b0.ids, "trans_l1", "both", True, g_pos, None)
    want = ref.grad(widened(ent), widened(rel), *pick(b0.np), "trans_l1", "both", True, 8, widened(g_pos)[sel], None)
    assert all(np_same(g[sel], w) for g, w in zip(got[:3], want[:3])) and got[3].shape == (b, 0, d)


# ---- B: gradient bits ------------------------------------------------------------------------
def upstream(torch, gen, k, corrupt):
    kp = 2 * k if corrupt == "both" else k
    return draw(torch, gen, (B,), torch.float32), (draw(torch, gen, (B, kp), torch.float32) if k else None)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("S", ["f32", "bf16", "f32-f16"])
def test_gradients_have_the_bits_of_the_restatement(torch, batches, S, d):
    """the kernel's rows == the restatement's; ent.grad / rel.grad == ops.scatter_add of the
    restatement's rows at [src | dst | neg] / rel_id (ids that name no row: key -1), rounded once"""
    from euler_amd import ops
    SE, SR = pairs(torch)[S]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(300 + d)
    ent, rel = draw(torch, gen, (ENT, d), SE), draw(torch, gen, (REL, d), SR)
    v = width(ent, rel)
    i = DIMS.index(d)
    for j, (kind, normalize, k) in enumerate((kind, nz, k) for kind in KINDS for nz in (True, False) for k in (0, 1, 5)):
        corrupt = CORRUPTS[(i + j) % 3] if k else "both"
        bt = batches[k]
        g_pos, g_neg = upstream(torch, gen, k, corrupt)
        tag = (kind, corrupt, normalize, k)
        got = ops._triple_score_grad_raw(ent, rel, *bt.ids, kind, corrupt, normalize, g_pos, g_neg)
        want = ref.grad(widened(ent), widened(rel), *bt.np, kind, corrupt, normalize, v, widened(g_pos),
                        None if g_neg is None else widened(g_neg))
        for g, w, name in zip(got, want, ("src", "rel", "dst", "neg")):
            assert np_same(g, w), tag + (name,)
        if j % 3 != i % 3:
            continue                                          # the autograd path: one K per (kind, normalize)
        e, r = ent.clone().requires_grad_(), rel.clone().requires_grad_()
        out = ops.triple_score(e, r, *bt.ids, kind=kind, corrupt=corrupt, normalize=normalize)
        loss = (out * g_pos).sum() if k == 0 else (out[0] * g_pos).sum() + (out[1] * g_neg).sum()
        loss.backward()
        rows = np.concatenate([want[0], want[2]] + ([want[3].reshape(-1, d)] if k else []))
        keys = bt.ent_keys()
        keys = np.where((keys >= 0) & (keys < ENT), keys, -1).astype(np.int32)
        want_ent = ops.scatter_add(torch.from_numpy(rows).cuda(), torch.from_numpy(keys).cuda(), ENT).to(SE)
        rkeys = np.where((bt.np[1] >= 0) & (bt.np[1] < REL), bt.np[1], -1).astype(np.int32)
        want_rel = ops.scatter_add(torch.from_numpy(want[1]).cuda(), torch.from_numpy(rkeys).cuda(), REL).to(SR)
        assert same(e.grad, want_ent) and same(r.grad, want_rel), tag
        assert e.grad.dtype == SE and r.grad.dtype == SR


@pytest.mark.parametrize("S", ["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_sparse_grad_equals_the_dense_gradient_on_its_rows(torch, batches, S, kind):
    from euler_amd import ops
    SE, SR = pairs(torch)[S]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    d = 20
    ent, rel = draw(torch, gen, (ENT, d), SE), draw(torch, gen, (REL, d), SR)
    bt = batches[5]
    g_pos, g_neg = upstream(torch, gen, 5, "both")
    grads = {}
    for sparse in (False, True):
        e, r = ent.clone().requires_grad_(), rel.clone().requires_grad_()
        pos, neg = ops.triple_score(e, r, *bt.ids, kind=kind, sparse_grad=sparse)
        ((pos * g_pos).sum() + (neg * g_neg).sum()).backward()
        grads[sparse] = (e.grad, r.grad)
    for (dense, sp), keys, rows in zip(zip(*[grads[False], grads[True]]), (bt.ent_keys(), bt.np[1]), (ENT, REL)):
        assert sp.is_sparse and sp.shape == dense.shape and sp.dtype == dense.dtype
        sp = sp.coalesce()
        idx = sp.indices()[0]
        looked_up = np.unique(keys[(keys >= 0) & (keys < rows)])
        assert np.array_equal(idx.cpu().numpy(), looked_up)               # absent elsewhere
        assert same(sp.values(), dense[idx])
        rest = torch.ones(rows, dtype=torch.bool, device="cuda")
        rest[idx] = False
        assert not bool(dense[rest].any())


def test_sparse_grad_of_ids_that_name_no_row(torch):
    from euler_amd import ops
    ent = torch.ones((4, 8), device="cuda", requires_grad=True)
    rel = torch.ones((2, 8), device="cuda", requires_grad=True)
    bad = torch.tensor([-1, 9, (1 << 33) + 5], device="cuda")
    pos, neg = ops.triple_score(ent, rel, bad, bad, bad, bad.reshape(3, 1), sparse_grad=True)
    (pos.sum() + neg.sum()).backward()
    for g in (ent.grad, rel.grad):
        assert g.is_sparse and g.coalesce().indices().numel() == 0 and g.shape in ((4, 8), (2, 8))
    assert bool((pos == 0).all()) and bool((neg == 0).all())


def test_repeated_ids_accumulate_and_bad_ids_get_nothing(torch, batches):
    """triples 4, 5, 6 share src[4] as src, src, dst, and negative (4, 0) is src[4] too"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    d = 64
    ent, rel = draw(torch, gen, (ENT, d), torch.float32), draw(torch, gen, (REL, d), torch.float32)
    bt = batches[5]
    g_pos, g_neg = upstream(torch, gen, 5, "both")
    gs, gr, gd, gn = ops._triple_score_grad_raw(ent, rel, *bt.ids, "trans_l1", "both", True, g_pos, g_neg)
    for rows, ids, n_rows in ((gs, bt.src, ENT), (gd, bt.dst, ENT), (gr, bt.rel_id, REL), (gn, bt.neg, ENT)):
        off = (ids < 0) | (ids >= n_rows)
        assert int(off.sum()) >= 1 and not bool(rows[off].any()) and bool(rows[~off].any(-1).all())
    e = ent.clone().requires_grad_()
    pos, neg = ops.triple_score(e, rel, *bt.ids, kind="trans_l1")
    ((pos * g_pos).sum() + (neg * g_neg).sum()).backward()
    node = int(bt.src[4])
    keys = torch.from_numpy(bt.ent_keys()).cuda()
    rows = torch.cat([gs, gd, gn.reshape(-1, d)])
    at = (keys == node).nonzero().reshape(-1)
    assert at.numel() >= 4
    acc = torch.zeros(d, device="cuda")
    for p in at.tolist():                                     # the occurrence order [src | dst | neg]
        acc = acc + rows[p]
    assert same(e.grad[node], acc)


# ---- C: the float64 composition --------------------------------------------------------------
def composition64(torch, ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize):
    """the reference's expressions in torch float64: lookup (an id that names no row: zeros),
    tf.nn.l2_normalize, the tile of the true triple, calculate_scores, the concat"""
    eps = float(np.float32(1e-12))

    def look(table, ids):
        ok = (ids >= 0) & (ids < table.shape[0])
        return table[ids.clamp(0, table.shape[0] - 1)] * ok.unsqueeze(-1)

    def norm(x):
        return x * torch.rsqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=eps)) if normalize else x

    def score(a, r, c):
        if kind == "distmult":
            return (a * r * c).sum(-1)
        e = a + r - c
        return -(e.abs().sum(-1) if kind == "trans_l1" else torch.linalg.vector_norm(e, dim=-1))

    h, r, t = norm(look(ent, src)), norm(look(rel, rel_id)), norm(look(ent, dst))
    pos = score(h, r, t)
    if neg is None:
        return pos, None
    n = norm(look(ent, neg))
    hh, rr, tt = (x.unsqueeze(1).expand_as(n) for x in (h, r, t))
    front, tail = score(n, rr, tt), score(hh, rr, n)
    return pos, front if corrupt == "front" else tail if corrupt == "tail" else torch.cat([front, tail], 1)


# (unit roundoff, half the spacing of the subnormals) of the dtype a table gradient is rounded to
UNIT = {"f32": (0.0, 0.0), "bf16": (2.0 ** -8, 0.0), "f16": (2.0 ** -11, 2.0 ** -25)}


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("S", ["f32", "bf16", "f16"])
def test_within_the_derived_bounds_of_the_float64_composition(torch, batches, S, d, capsys):
    """forward: gamma(n(kind, d)) * sum of magnitudes; table gradients: the propagated bound of
    triple_score_ref (GRAD_BOUND_NOTES), plus the one rounding of a 16-bit gradient; no margin.
    16-bit tables are compared on their widened values."""
    from euler_amd import ops
    SE, SR = pairs(torch)[S]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(400 + d)
    ent, rel = draw(torch, gen, (ENT, d), SE), draw(torch, gen, (REL, d), SR)
    i = DIMS.index(d)
    worst_f = worst_g = 0.0
    for j, (kind, normalize) in enumerate((kind, nz) for kind in KINDS for nz in (True, False)):
        k = (5, 1)[(i + j) % 2]
        corrupt = CORRUPTS[(i + j) % 3]
        bt = batches[k]
        g_pos, g_neg = upstream(torch, gen, k, corrupt)
        e, r = ent.clone().requires_grad_(), rel.clone().requires_grad_()
        pos, neg = ops.triple_score(e, r, *bt.ids, kind=kind, corrupt=corrupt, normalize=normalize)
        ((pos * g_pos).sum() + (neg * g_neg).sum()).backward()
        e64, r64 = ent.double().requires_grad_(), rel.double().requires_grad_()
        p64, n64 = composition64(torch, e64, r64, *bt.ids, kind, corrupt, normalize)
        ((p64 * g_pos.double()).sum() + (n64 * g_neg.double()).sum()).backward()
        tag = (kind, corrupt, normalize, k)
        # forward
        _, _, mag_pos, mag_neg = ref.forward64(widened(ent), widened(rel), *bt.np, kind, corrupt, normalize)
        for got, want, mag in ((pos, p64, mag_pos), (neg, n64, mag_neg)):
            err = (got.detach().double() - want.detach()).abs().cpu().numpy()
            bound = ref.forward_bound(kind, d, mag)
            assert np.all(err <= bound), tag
            worst_f = max(worst_f, float(np.max(err / np.maximum(bound, 1e-300))))
        # table gradients
        (gs, bs), (gr, br), (gd, bd), (gn, bn) = ref.grad64(widened(ent), widened(rel), *bt.np, kind, corrupt,
                                                            normalize, widened(g_pos), widened(g_neg))
        t_ent, b_ent = ref.table_grad64(np.concatenate([gs, gd, gn.reshape(-1, d)]),
                                        np.concatenate([bs, bd, bn.reshape(-1, d)]), bt.ent_keys(), ENT,
                                        *UNIT[S])
        t_rel, b_rel = ref.table_grad64(gr, br, bt.np[1], REL, *UNIT[S])
        for got, want, center, bound in ((e.grad, e64.grad, t_ent, b_ent), (r.grad, r64.grad, t_rel, b_rel)):
            want = want.cpu().numpy()
            known = np.isfinite(bound)
            assert np.all(np.abs(want - center)[known] <= 1e-9 * (1 + np.abs(center[known]))), tag   # the two float64 forms agree
            err = np.abs(got.double().cpu().numpy() - want)
            assert np.all(err <= bound), tag + (float(np.max(err / np.maximum(bound, 1e-300))),)
            worst_g = max(worst_g, float(np.max(err / np.maximum(bound, 1e-300))))
    with capsys.disabled():
        print("\n[triple_score %s d=%d] worst error / bound: forward %.4f, table gradients %.4f"
              % (S, d, worst_f, worst_g))
    assert 0 < worst_f <= 1 and 0 < worst_g <= 1


# ---- D: captured graph -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["trans_l2", "distmult"])
def test_both_entries_replay_from_a_captured_graph(torch, batches, kind):
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    d = 128
    ent, rel = draw(torch, gen, (ENT, d), torch.bfloat16), draw(torch, gen, (REL, d), torch.float32)
    bt = batches[5]
    g_pos, g_neg = upstream(torch, gen, 5, "both")
    want = ops.triple_score(ent, rel, *bt.ids, kind=kind)
    want_g = ops._triple_score_grad_raw(ent, rel, *bt.ids, kind, "both", True, g_pos, g_neg)
    v = width(ent, rel)
    assert np_same(want[0], ref.forward(widened(ent), widened(rel), *bt.np, kind, "both", True, v)[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.triple_score(ent, rel, *bt.ids, kind=kind)                                        # (warm up)
        ops._triple_score_grad_raw(ent, rel, *bt.ids, kind, "both", True, g_pos, g_neg)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = ops.triple_score(ent, rel, *bt.ids, kind=kind)
            out_g = ops._triple_score_grad_raw(ent, rel, *bt.ids, kind, "both", True, g_pos, g_neg)
        for _ in range(2):
            for t in out + out_g:
                t.zero_()
            g.replay()
            side.synchronize()
            assert all(same(a, b) for a, b in zip(out + out_g, want + want_g))
    torch.cuda.current_stream().wait_stream(side)


# ---- E: the C entries ------------------------------------------------------------------------
GUARD = -12345.0


class Call(object):
    """euler_gpu_triple_score / _grad on small buffers with 4 guard words behind every output"""

    def __init__(self, torch):
        from euler_amd import _lib
        self.torch, self.lib = torch, _lib
        self.b, self.k, self.d = 6, 3, 8
        b, k, d = self.b, self.k, self.d
        self.ent = torch.ones((32, d), device="cuda")
        self.rel = torch.ones((4, d), device="cuda")
        self.ids = torch.arange(b, device="cuda")
        self.neg = torch.arange(b * k, device="cuda").reshape(b, k)
        self.g = torch.ones(b * 2 * k, device="cuda")
        self.sizes = dict(pos=b, neg_out=b * 2 * k, g_src=b * d, g_rel=b * d, g_dst=b * d, g_neg_rows=b * k * d)
        self.out = {n: torch.full((s + 4,), GUARD, device="cuda") for n, s in self.sizes.items()}

    def p(self, t):
        return C.c_void_p(t.data_ptr())

    def head(self, a):
        return (a["kind"], a["normalize"], a["corrupt"], a["ent"], a["ent_dt"], a["ent_rows"], a["rel"], a["rel_dt"],
                a["rel_rows"], a["src"], a["rel_id"], a["dst"], a["neg"], a["b"], a["k"], a["d"])

    def base(self):
        base = dict(kind=0, normalize=1, corrupt=2, ent=self.p(self.ent), ent_dt=self.lib.F32, ent_rows=32,
                    rel=self.p(self.rel), rel_dt=self.lib.F32, rel_rows=4, src=self.p(self.ids), rel_id=self.p(self.ids),
                    dst=self.p(self.ids), neg=self.p(self.neg), b=self.b, k=self.k, d=self.d,
                    g_pos=self.p(self.g), g_neg=self.p(self.g))
        base.update({n: self.p(t) for n, t in self.out.items()})
        return base

    def forward(self, **kw):
        from euler_amd.ops import _stream
        a = dict(self.base(), **kw)
        rc = self.lib.lib().euler_gpu_triple_score(_stream(), *self.head(a), a["pos"], a["neg_out"])
        self.torch.cuda.synchronize()
        return rc

    def grad(self, **kw):
        from euler_amd.ops import _stream
        a = dict(self.base(), **kw)
        rc = self.lib.lib().euler_gpu_triple_score_grad(_stream(), *self.head(a), a["g_pos"], a["g_neg"], a["g_src"],
                                                       a["g_rel"], a["g_dst"], a["g_neg_rows"])
        self.torch.cuda.synchronize()
        return rc

    def untouched(self, *names):
        return all(bool((self.out[n] == GUARD).all()) for n in (names or self.out))


def test_c_entry_error_rules(torch):
    c = Call(torch)
    EINVAL = c.lib.EINVAL
    for call in (c.forward, c.grad):
        assert call(kind=-1) == EINVAL and call(kind=3) == EINVAL
        assert call(corrupt=-1) == EINVAL and call(corrupt=3) == EINVAL
        assert call(ent_dt=3) == EINVAL and call(rel_dt=-1) == EINVAL
        assert call(k=-1) == EINVAL
        assert call(neg=None) == EINVAL                                   # k > 0 without negatives
        assert call(ent_rows=0) == EINVAL and call(rel_rows=0) == EINVAL
        assert call(b=1 << 30) == EINVAL                                  # b * max(k, 1) * 2 >= 2^31
        assert call(b=1 << 30, k=0) == EINVAL
        assert call(b=1 << 20, k=1 << 10) == EINVAL
        assert call(d=1 << 31) == EINVAL
        for name in ("ent", "rel", "src", "rel_id", "dst"):
            assert call(**{name: None}) == EINVAL, name
    assert c.forward(pos=None) == EINVAL and c.forward(neg_out=None) == EINVAL
    for name in ("g_pos", "g_neg", "g_src", "g_rel", "g_dst", "g_neg_rows"):
        assert c.grad(**{name: None}) == EINVAL, name
    assert c.untouched()


def test_c_entry_empty_shapes_and_guard_words(torch):
    c = Call(torch)
    OK = c.lib.OK
    # b == 0 or d == 0: OK, nothing touched - null buffers included
    assert c.forward(b=0) == OK and c.grad(b=0) == OK and c.forward(d=0) == OK and c.grad(d=0) == OK
    assert c.forward(b=0, ent=None, src=None, pos=None) == OK and c.grad(d=0, g_src=None, g_pos=None) == OK
    assert c.untouched()
    # k == 0: the negative outputs stay untouched (and may be null)
    assert c.forward(k=0) == OK and c.grad(k=0) == OK
    assert c.untouched("neg_out", "g_neg_rows")
    assert not bool((c.out["pos"][:c.b] == GUARD).any()) and bool((c.out["pos"][c.b:] == GUARD).all())
    assert c.forward(k=0, neg=None, neg_out=None) == OK and c.grad(k=0, neg=None, g_neg=None, g_neg_rows=None) == OK
    # the full call writes exactly [B] / [B, K'] / [B, d] / [B, K, d]
    for corrupt, kp in ((0, c.k), (1, c.k), (2, 2 * c.k)):
        c2 = Call(torch)
        assert c2.forward(corrupt=corrupt) == OK and c2.grad(corrupt=corrupt) == OK
        sizes = dict(c2.sizes, neg_out=c2.b * kp)
        for n, s in sizes.items():
            assert not bool((c2.out[n][:s] == GUARD).any()) and bool((c2.out[n][s:] == GUARD).all()), (corrupt, n)


def test_python_argument_checks(torch):
    from euler_amd import ops
    ent, rel = torch.ones((4, 8), device="cuda"), torch.ones((2, 8), device="cuda")
    i = torch.zeros(3, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        ops.triple_score(ent, rel, i, i, i, kind="transh")
    with pytest.raises(ValueError):
        ops.triple_score(ent, rel, i, i, i, corrupt="head")
    with pytest.raises(ValueError):
        ops.triple_score(ent, torch.ones((2, 4), device="cuda"), i, i, i)
    with pytest.raises(ValueError):
        ops.triple_score(ent, rel, i, i[:2], i)
    with pytest.raises(TypeError):
        ops.triple_score(ent.double(), rel, i, i, i)
    with pytest.raises(RuntimeError):
        ops.triple_score(ent.cpu(), rel, i, i, i)
    empty = ops.triple_score(ent, rel, i[:0], i[:0], i[:0], i[:0].reshape(0, 5))
    assert empty[0].shape == (0,) and empty[1].shape == (0, 10)
    none = ops.triple_score(ent[:, :0], rel[:, :0], i, i, i, i.reshape(3, 1))
    assert none[0].shape == (3,) and not bool(none[0].any()) and none[1].shape == (3, 2)


# ---- F: the example's step -------------------------------------------------------------------
@pytest.fixture(scope="module")
def example():
    spec = importlib.util.spec_from_file_location(
        "transe_minibatch", os.path.join(ROOT, "examples", "python", "transe_minibatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("kind", KINDS)
def test_example_step_on_the_fixture_graph(torch, example, kind):
    """the fused loss and the composed loss agree within the forward bound of C carried through
    the loss (the mean over K', the clamp and the mean over B are 1-Lipschitz averages, each with
    its own roundings); one SparseAdam step changes exactly the rows that were looked up"""
    import euler_amd
    G = euler_amd.Graph.load(FIXTURE, edges=True)
    G.set_seed(7)
    batch, negs, d = 64, 5, 32
    n_ent, n_rel = G.id_range()[0] + 1, G.num_edge_types
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    ent0, rel0 = draw(torch, gen, (n_ent, d), torch.float32), draw(torch, gen, (n_rel, d), torch.float32)
    src, rel_id, dst, neg = example.sample_batch(G, batch, negs)
    assert bool(((rel_id >= 0) & (rel_id < n_rel)).all()) and bool(((neg >= 0) & (neg < n_ent)).all())
    losses, tables = {}, {}
    for composed in (False, True):
        ent, rel = torch.nn.Parameter(ent0.clone()), torch.nn.Parameter(rel0.clone())
        opt = torch.optim.SparseAdam([ent, rel], lr=0.01)
        pos, scores = example.energies(ent, rel, src, rel_id, dst, neg, kind, composed)
        loss = example.margin_loss(pos, scores)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses[composed], tables[composed] = float(loss), (ent.detach(), rel.detach())
        assert 0 < float(example.mrr(pos.detach(), scores.detach())) <= 1
    # the bound: per score gamma(n) * mag (C), on both sides of a float64 truth; the loss adds the
    # roundings of margin + mean - pos (2 K' + 2 operations) and of the mean over B (B operations)
    ids = [t.cpu().numpy() for t in (src, rel_id, dst, neg)]
    p64, n64, mag_pos, mag_neg = ref.forward64(widened(ent0), widened(rel0), *ids, kind, "both", True)
    per_triple = ref.forward_bound(kind, d, mag_pos) + ref.forward_bound(kind, d, mag_neg).mean(1)
    size = 1.0 + np.abs(n64).mean(1) + np.abs(p64) + per_triple
    bound = 2 * (per_triple.mean() + ref.gamma(2 * 2 * negs + 2 + batch) * size.mean())
    print("\n[transe example %s] fused %.9g composed %.9g |diff| / bound = %.4f"
          % (kind, losses[False], losses[True], abs(losses[False] - losses[True]) / bound))
    assert abs(losses[False] - losses[True]) <= bound
    # exactly the looked-up rows moved (SparseAdam moves every row its gradient names)
    for t, (before, keys) in enumerate(((ent0, np.concatenate([ids[0], ids[2], ids[3].reshape(-1)])), (rel0, ids[1]))):
        for composed in (False, True):
            moved = (tables[composed][t] != before).any(1).cpu().numpy()
            want = np.zeros(before.shape[0], bool)
            want[keys] = True
            assert np.array_equal(moved, want), (kind, composed, t)


@pytest.mark.parametrize("mode", [[], ["--composed"]])
def test_example_runs(mode):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", "transe_minibatch.py"),
                        "--kind", "trans_l2"] + mode, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "loss" in r.stdout and ("composed" in r.stdout) == bool(mode), r.stdout
