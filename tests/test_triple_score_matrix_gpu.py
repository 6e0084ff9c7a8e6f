"""Triple scoring with TransR's matrix projection on the GPU (ops.triple_score_matrix,
euler_gpu_triple_score_matrix[_grad]):
  A  forward bits == the numpy restatement tests/triple_score_matrix_ref.py (dims, the cap, dtypes,
     unaligned views, the grid stride)
  B  per-occurrence gradient bits == the restatement; the ent / rel gradients == ops.scatter_add of
     those rows in occurrence order; the matrix gradient == the ordered restatement; sparse_grad
  C  the grouping: one relation, every triple its own relation, unused relations, bad rel_ids,
     permutations of the batch, a relation's triples alone
  D  the peak allocation of forward + backward stays below one matrix per triple
  E  both entries replay from a captured graph; the rules of the C entries; empty shapes; guard
     words; the Python argument checks; the example's step, fused against --composed"""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import triple_score_matrix_ref as ref

pytestmark = pytest.mark.gpu

ENT, REL, B = 300, 7, 90
KINDS, CORRUPTS = ("trans_l1", "trans_l2"), ("front", "tail", "both")
FIXTURE = os.path.join(ROOT, "tests", "golden", "fixture_dat")
NAMES = ("src", "rel", "dst", "neg", "gz_src", "gz_dst", "gz_neg")
CAP = (ref.MAX_DIM, ref.MAX_DIM)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def triples(torch):
    """storage dtypes of (ent, rel, matrix)"""
    f, b, h = torch.float32, torch.bfloat16, torch.float16
    return {"f32": (f, f, f), "bf16": (b, b, b), "f16": (h, h, h), "bf16-f32-f16": (b, f, h), "f32-f16-bf16": (f, h, b)}


def draw(torch, gen, shape, S, unaligned=False, scale=4.0):
    """values of dtype S in [-scale, scale]; unaligned: a view that starts ONE ELEMENT into its storage"""
    x = ((torch.rand(shape, generator=gen, device="cuda") * 2 - 1) * scale).to(S)
    if unaligned:
        buf = torch.empty(x.numel() + 1, dtype=S, device="cuda")
        buf[1:] = x.reshape(-1)
        x = buf[1:].view(shape)
        assert x.data_ptr() % 16 == x.element_size() and x.is_contiguous()
    return x


class Tabs(object):
    """ent [ent_rows, de], rel [rel_rows, dr], matrix [rel_rows, de * dr] in the storage triple S"""

    def __init__(self, torch, gen, de, dr, S="f32", unaligned=(), ent_rows=ENT, rel_rows=REL):
        SE, SR, SM = triples(torch)[S] if isinstance(S, str) else S
        self.ent = draw(torch, gen, (ent_rows, de), SE, "ent" in unaligned)
        self.rel = draw(torch, gen, (rel_rows, dr), SR, "rel" in unaligned)
        self.matrix = draw(torch, gen, (rel_rows, de * dr), SM, "matrix" in unaligned, scale=1.0)
        self.all = (self.ent, self.rel, self.matrix)
        self.np = tuple(t.float().cpu().numpy() for t in self.all)
        self.v = ref.matrix_chunk_width(dr, self.rel.data_ptr(), self.rel.element_size())


class Batch(object):
    """b triples with k negatives: ids repeat inside the batch, a negative equals its src, and
    (bad) some ids name no row (-1, rows + 3, 2^33 + 5), in each of the three roles"""

    def __init__(self, torch, k, seed=3, b=B, bad=True, ent_rows=ENT, rel_rows=REL, rel_id=None):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed + k)
        r = lambda hi, shape: torch.randint(0, hi, shape, generator=gen, device="cuda")      # noqa: E731
        self.k, self.b = k, b
        self.src, self.dst, self.rel_id = r(ent_rows, (b,)), r(ent_rows, (b,)), r(rel_rows, (b,))
        if rel_id is not None:
            self.rel_id = rel_id
        self.neg = r(ent_rows, (b, k)) if k else None
        if b > 16:
            self.src[5] = self.src[4]
            self.dst[6] = self.src[4]
            if bad:
                self.src[10], self.dst[11], self.rel_id[12] = -1, ent_rows + 3, (1 << 33) + 5
                self.src[13], self.rel_id[14], self.rel_id[9] = (1 << 33) + 5, -1, rel_rows + 3
            if k:
                self.neg[4, 0] = self.src[4]
                if bad:
                    self.neg[15, 0], self.neg[16, k - 1] = -1, ent_rows + 3
        self.freeze()

    def freeze(self):
        self.ids = (self.src, self.rel_id, self.dst, self.neg)
        self.np = [None if t is None else t.cpu().numpy() for t in self.ids]

    def take(self, torch, sel):
        """the triples `sel` (an index tensor), in that order"""
        out = Batch.__new__(Batch)
        out.k, out.b = self.k, int(sel.numel())
        out.src, out.rel_id, out.dst = self.src[sel], self.rel_id[sel], self.dst[sel]
        out.neg = None if self.neg is None else self.neg[sel]
        out.freeze()
        return out

    def ent_keys(self):
        return np.concatenate([self.np[0], self.np[2]] + ([self.np[3].reshape(-1)] if self.k else []))


@pytest.fixture(scope="module")
def batches(torch):
    return {k: Batch(torch, k) for k in (0, 1, 5)}


def np_same(got, want):
    got = got.cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


def same(a, b):
    """two device tensors, bit for bit"""
    import torch
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    w = torch.int32 if a.element_size() == 4 else torch.int16
    return bool(torch.equal(a.contiguous().view(w), b.contiguous().view(w)))


def upstream(torch, gen, k, corrupt, b=B):
    kp = 2 * k if corrupt == "both" else k
    return draw(torch, gen, (b,), torch.float32), (draw(torch, gen, (b, kp), torch.float32) if k else None)


def fwd(ops, t, bt, kind, corrupt):
    return ops.triple_score_matrix(*t.all, *bt.ids, kind=kind, corrupt=corrupt)


def raw_grad(torch, ops, t, bt, kind, corrupt, g_pos, g_neg, segments="dense"):
    """the C entry through ops._triple_score_matrix_grad_raw with the grouping ops builds"""
    order, keys = ops._matrix_grouping(bt.rel_id, t.rel.shape[0])
    seg_ptr, seg_rel = (None, None) if segments is None else ops._matrix_segments(keys, t.rel.shape[0], False)
    return ops._triple_score_matrix_grad_raw(*t.all, *bt.ids, kind, corrupt, order, seg_ptr, seg_rel, g_pos, g_neg)


def want_grad(torch, t, bt, kind, corrupt, g_pos, g_neg, with_matrix=True):
    """the restatement: the seven row blocks and G_M rounded once to the matrix's dtype"""
    wide = lambda x: None if x is None else x.float().cpu().numpy()                      # noqa: E731
    rows = ref.grad(*t.np, *bt.np, kind, corrupt, t.v, wide(g_pos), wide(g_neg))
    if not with_matrix:
        return rows, None
    gm = ref.matrix_grad(t.np[0], t.rel.shape[0], *bt.np, rows[4], rows[5], rows[6])
    return rows, torch.from_numpy(gm).to(t.matrix.dtype).cuda()


def check_forward(torch, ops, t, bt, kind, corrupt):
    got = fwd(ops, t, bt, kind, corrupt)
    want_pos, want_neg = ref.forward(*t.np, *bt.np, kind, corrupt, t.v)
    tag = (kind, corrupt, bt.k, t.v)
    if bt.k == 0:
        assert torch.is_tensor(got) and np_same(got, want_pos), tag
    else:
        assert np_same(got[0], want_pos) and np_same(got[1], want_neg), tag
        assert got[1].shape == (bt.b, 2 * bt.k if corrupt == "both" else bt.k)
    return got


def check_grad(torch, ops, t, bt, kind, corrupt, gen):
    g_pos, g_neg = upstream(torch, gen, bt.k, corrupt, bt.b)
    got = raw_grad(torch, ops, t, bt, kind, corrupt, g_pos, g_neg)
    want, want_gm = want_grad(torch, t, bt, kind, corrupt, g_pos, g_neg)
    for g, w, name in zip(got, want, NAMES):
        assert np_same(g, w), (kind, corrupt, bt.k, t.v, name)
    assert same(got[7], want_gm), (kind, corrupt, bt.k, "matrix")
    return got, want, want_gm, g_pos, g_neg


def configs(i, full):
    """(kind, corrupt, K): the full cross, or K in 0, 1, 5 with the rest rotating"""
    if full:
        return [(kind, c, k) for kind in KINDS for k in (0, 1, 5) for c in (CORRUPTS if k else ("both",))]
    return [(KINDS[(i + j) % 2], CORRUPTS[(i + j) % 3] if k else "both", k) for j, k in enumerate((0, 1, 5))]


# ---- A: forward bits -------------------------------------------------------------------------
@pytest.mark.parametrize("de,dr", ref.DIMS)
@pytest.mark.parametrize("S", ["f32", "bf16", "f16", "bf16-f32-f16", "f32-f16-bf16"])
def test_forward_has_the_bits_of_the_restatement(torch, batches, S, de, dr):
    """(17, 65) crosses the 16-row and 64-column tiles of the gradient kernels, (100, 100) and
    (130, 70) the LDS tile of the per-triple kernels (8192 / dr rows of M)"""
    from euler_amd import ops
    i = ref.DIMS.index((de, dr))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(100 + i)
    t = Tabs(torch, gen, de, dr, S)
    assert t.v == (8 if dr % 8 == 0 else 4 if dr % 4 == 0 else 1)
    for kind, corrupt, k in configs(i, (de, dr) in ((3, 5), (32, 32), (100, 100))):
        check_forward(torch, ops, t, batches[k], kind, corrupt)


@pytest.mark.parametrize("S", ["f32", "bf16-f32-f16"])
def test_forward_and_gradient_at_the_cap(torch, S):
    """de = dr = 512 with B = 3 and two relations; one past the cap is refused"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    t = Tabs(torch, gen, *CAP, S, rel_rows=2)
    bt = Batch(torch, 5, b=3, rel_rows=2)
    check_forward(torch, ops, t, bt, "trans_l2", "both")
    check_grad(torch, ops, t, bt, "trans_l1", "both", gen)
    for de, dr in ((CAP[0] + 1, 8), (8, CAP[1] + 1)):
        big = Tabs(torch, gen, de, dr, "f32", rel_rows=2)
        with pytest.raises(ValueError):
            fwd(ops, big, bt, "trans_l1", "both")


@pytest.mark.parametrize("de,dr", [(8, 8), (32, 32), (100, 100)])
@pytest.mark.parametrize("S", ["f32", "bf16", "bf16-f32-f16"])
def test_forward_and_gradient_on_unaligned_views(torch, batches, S, de, dr):
    """every table as a view that starts one element into its storage: only rel's start decides V"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(200 + de)
    bt = batches[5]
    for j, off in enumerate((("ent", "rel", "matrix"), ("rel",), ("ent",), ("matrix",))):
        t = Tabs(torch, gen, de, dr, S, unaligned=off)
        assert t.v == (1 if "rel" in off else 8 if dr % 8 == 0 else 4)
        check_forward(torch, ops, t, bt, KINDS[j % 2], "both")
        check_grad(torch, ops, t, bt, KINDS[(j + 1) % 2], "both", gen)


def test_grid_stride(torch):
    """de = dr = 1 gives 256 triples a workgroup and the launcher caps the grid at 2048
    workgroups: with B = 256 * 2048 + 300 the last 300 triples of the grouped order are a
    workgroup's second share (the gx kernel, 16 triples a share, strides 17 times).  Triples are
    independent: the restatement is taken for a sample, the rest is held against a second call."""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    b = 256 * 2048 + 300
    t = Tabs(torch, gen, 1, 1)
    bt = Batch(torch, 0, seed=40, b=b)
    order, _ = ops._matrix_grouping(bt.rel_id, REL)
    sel = torch.cat([torch.arange(64, device="cuda"), order[:64], order[-364:]])
    pos = fwd(ops, t, bt, "trans_l1", "both")
    part = bt.take(torch, sel)
    assert pos.shape == (b,) and np_same(pos[sel], ref.forward(*t.np, *part.np, "trans_l1", "both", 1)[0])
    assert same(pos, fwd(ops, t, bt, "trans_l1", "both"))
    g_pos = draw(torch, gen, (b,), torch.float32)
    got = raw_grad(torch, ops, t, bt, "trans_l1", "both", g_pos, None, segments=None)
    again = raw_grad(torch, ops, t, bt, "trans_l1", "both", g_pos, None, segments=None)
    want, _ = want_grad(torch, t, part, "trans_l1", "both", g_pos[sel], None, with_matrix=False)
    for g, g2, w, name in zip(got, again, want, NAMES):
        if name in ("neg", "gz_neg"):
            assert g.shape[:2] == (b, 0)
        else:
            assert np_same(g[sel], w) and same(g, g2), name
    assert got[7] is None


# ---- B: gradient bits ------------------------------------------------------------------------
def scattered(torch, ops, rows, keys, n_rows, dt):
    keys = np.where((keys >= 0) & (keys < n_rows), keys, -1).astype(np.int32)
    return ops.scatter_add(torch.from_numpy(rows).cuda(), torch.from_numpy(keys).cuda(), n_rows).to(dt)


@pytest.mark.parametrize("de,dr", ref.DIMS)
@pytest.mark.parametrize("S", ["f32", "bf16", "f32-f16-bf16"])
def test_gradients_have_the_bits_of_the_restatement(torch, batches, S, de, dr):
    """the kernels' rows (gx, g_rel, gz) == the restatement's; G_M == the ordered restatement,
    rounded once; through autograd the gradient of ent / rel == ops.scatter_add of the
    restatement's rows at [src | dst | neg] / rel_id and the gradient of matrix == G_M"""
    from euler_amd import ops
    i = ref.DIMS.index((de, dr))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(300 + i)
    t = Tabs(torch, gen, de, dr, S)
    for j, (kind, corrupt, k) in enumerate(configs(i, (de, dr) in ((3, 5), (64, 33)))):
        bt = batches[k]
        got, want, want_gm, g_pos, g_neg = check_grad(torch, ops, t, bt, kind, corrupt, gen)
        if j % 3 != i % 3:
            continue                                          # the autograd path: one K per (de, dr)
        params = [x.clone().requires_grad_() for x in t.all]
        if j % 2:
            params[2] = t.matrix.clone().reshape(REL, de, dr).requires_grad_()          # [R, de, dr] is accepted
        out = ops.triple_score_matrix(*params, *bt.ids, kind=kind, corrupt=corrupt)
        loss = (out * g_pos).sum() if k == 0 else (out[0] * g_pos).sum() + (out[1] * g_neg).sum()
        loss.backward()
        ent_rows = np.concatenate([want[0], want[2]] + ([want[3].reshape(-1, de)] if k else []))
        assert same(params[0].grad, scattered(torch, ops, ent_rows, bt.ent_keys(), ENT, t.ent.dtype))
        assert same(params[1].grad, scattered(torch, ops, want[1], bt.np[1], REL, t.rel.dtype))
        assert same(params[2].grad.reshape(REL, de * dr), want_gm)
        assert all(p.grad.dtype == p.dtype and p.grad.shape == p.shape for p in params)


@pytest.mark.parametrize("S", ["f32", "bf16"])
def test_sparse_grad_equals_the_dense_gradient_on_its_rows(torch, batches, S):
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    rel_rows = REL + 3                                                  # relations 7, 8, 9 have no triple
    t = Tabs(torch, gen, 20, 12, S, rel_rows=rel_rows)
    bt = batches[5]
    g_pos, g_neg = upstream(torch, gen, 5, "both")
    grads = {}
    for sparse in (False, True):
        params = [x.clone().requires_grad_() for x in t.all]
        pos, neg = ops.triple_score_matrix(*params, *bt.ids, kind="trans_l2", sparse_grad=sparse)
        ((pos * g_pos).sum() + (neg * g_neg).sum()).backward()
        grads[sparse] = [p.grad for p in params]
    for dense, sp, keys, rows in zip(grads[False], grads[True], (bt.ent_keys(), bt.np[1], bt.np[1]),
                                     (ENT, rel_rows, rel_rows)):
        assert sp.is_sparse and sp.shape == dense.shape and sp.dtype == dense.dtype
        sp = sp.coalesce()
        idx = sp.indices()[0]
        looked_up = np.unique(keys[(keys >= 0) & (keys < rows)])
        assert np.array_equal(idx.cpu().numpy(), looked_up)               # absent elsewhere
        assert same(sp.values(), dense[idx])
        rest = torch.ones(rows, dtype=torch.bool, device="cuda")
        rest[idx] = False
        assert int(rest.sum()) >= 1 and not bool(dense[rest].any())
    with pytest.raises(ValueError):
        ops.triple_score_matrix(t.ent, t.rel, t.matrix.reshape(rel_rows, 20, 12), *bt.ids, sparse_grad=True)
    if S != "f32":
        return
    opt_params = [torch.nn.Parameter(x.clone()) for x in t.all]          # SparseAdam takes all three
    opt = torch.optim.SparseAdam(opt_params, lr=0.01)
    pos, neg = ops.triple_score_matrix(*opt_params, *bt.ids, sparse_grad=True)
    (pos.sum() + neg.sum()).backward()
    opt.step()
    assert all(bool((p.detach() != x).any()) for p, x in zip(opt_params, t.all))


# ---- C: grouping -----------------------------------------------------------------------------
@pytest.mark.parametrize("b,de,dr,k", [(B, 20, 12, 5), (5000, 8, 8, 1), (1, 20, 12, 5)])
def test_all_triples_on_one_relation(torch, b, de, dr, k):
    """B = 5000 with de = dr = 8 crosses every staging batch of the matrix-gradient kernel (64
    occurrence rows) and every workgroup share of the per-triple kernels (256 triples); B = 1"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(41)
    t = Tabs(torch, gen, de, dr)
    bt = Batch(torch, k, seed=50, b=b, bad=False, rel_id=torch.full((b,), 3, dtype=torch.int64, device="cuda"))
    check_forward(torch, ops, t, bt, "trans_l2", "both")
    got = check_grad(torch, ops, t, bt, "trans_l1", "both", gen)[0]
    gm = got[7]
    assert bool(gm[3].any()) and not bool(gm[:3].any()) and not bool(gm[4:].any())
    assert not bool(torch.signbit(gm[0]).any())                           # an unused relation's row is +0


def test_every_triple_on_its_own_relation(torch):
    """B relations in a random order, and 20000 relations (more segments than grid rows) of which
    64 are used"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(42)
    t = Tabs(torch, gen, 20, 12, rel_rows=B)
    bt = Batch(torch, 5, seed=51, bad=False, rel_rows=B, rel_id=torch.randperm(B, generator=gen, device="cuda"))
    check_forward(torch, ops, t, bt, "trans_l1", "both")
    check_grad(torch, ops, t, bt, "trans_l2", "both", gen)
    many = 20000
    t = Tabs(torch, gen, 3, 3, rel_rows=many)
    rel_id = torch.randperm(many, generator=gen, device="cuda")[:64]
    bt = Batch(torch, 1, seed=52, b=64, bad=False, rel_rows=many, rel_id=rel_id)
    check_forward(torch, ops, t, bt, "trans_l2", "both")
    gm = check_grad(torch, ops, t, bt, "trans_l1", "both", gen)[0][7]
    used = torch.zeros(many, dtype=torch.bool, device="cuda")
    used[rel_id] = True
    assert bool(gm[used].any(1).all()) and not bool(gm[~used].any())


@pytest.mark.parametrize("kind", KINDS)
def test_rel_ids_that_name_no_relation(torch, kind):
    """-1, R + 3 and 2^33 + 5 mixed in: those triples lose rel[rho] and M_rho, their entity rows
    get zero gradients, and no matrix takes a term from them"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(43)
    t = Tabs(torch, gen, 20, 12)
    bt = Batch(torch, 5, seed=53, bad=False)
    bad = torch.tensor([-1, REL + 3, (1 << 33) + 5], device="cuda").repeat(10)
    at = torch.arange(0, B, 3, device="cuda")
    bt.rel_id[at] = bad
    bt.freeze()
    check_forward(torch, ops, t, bt, kind, "both")
    got = check_grad(torch, ops, t, bt, kind, "both", gen)[0]
    assert not any(bool(got[i][at].any()) for i in (0, 1, 2, 3))
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[at] = False
    rest = bt.take(torch, keep.nonzero().reshape(-1))
    g_pos, g_neg = upstream(torch, gen, 5, "both")
    whole = raw_grad(torch, ops, t, bt, kind, "both", g_pos, g_neg)[7]
    alone = raw_grad(torch, ops, t, rest, kind, "both", g_pos[keep], g_neg[keep])[7]
    assert same(whole, alone) and bool(whole.any())


@pytest.mark.parametrize("S", ["f32", "bf16"])
def test_permuting_the_batch_permutes_its_rows(torch, batches, S):
    """pos, neg and the per-occurrence rows follow their triples bit for bit, whatever the
    grouping does with them"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(44)
    t = Tabs(torch, gen, 33, 64, S)
    bt = batches[5]
    perm = torch.randperm(B, generator=gen, device="cuda")
    moved = bt.take(torch, perm)
    g_pos, g_neg = upstream(torch, gen, 5, "both")
    for kind in KINDS:
        pos, neg = fwd(ops, t, bt, kind, "both")
        pos2, neg2 = fwd(ops, t, moved, kind, "both")
        assert same(pos[perm], pos2) and same(neg[perm], neg2)
        rows = raw_grad(torch, ops, t, bt, kind, "both", g_pos, g_neg)
        rows2 = raw_grad(torch, ops, t, moved, kind, "both", g_pos[perm], g_neg[perm])
        for a, c, name in zip(rows[:7], rows2[:7], NAMES):
            assert same(a[perm], c), (kind, name)


@pytest.mark.parametrize("S", ["f32", "f32-f16-bf16"])
def test_a_relations_matrix_gradient_does_not_see_the_other_triples(torch, batches, S):
    """for each relation G_M[rho] from the whole batch == G_M[rho] from a call on that relation's
    triples alone, kept in their order"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(45)
    t = Tabs(torch, gen, 17, 65, S)
    bt = batches[5]
    g_pos, g_neg = upstream(torch, gen, 5, "both")
    whole = raw_grad(torch, ops, t, bt, "trans_l2", "both", g_pos, g_neg)[7]
    for rho in range(REL):
        at = (bt.rel_id == rho).nonzero().reshape(-1)
        assert at.numel() >= 2
        alone = raw_grad(torch, ops, t, bt.take(torch, at), "trans_l2", "both", g_pos[at], g_neg[at])[7]
        assert same(whole[rho], alone[rho]) and bool(whole[rho].any()), rho
        assert not bool(alone[:rho].any()) and not bool(alone[rho + 1:].any())


# ---- D: memory -------------------------------------------------------------------------------
def test_forward_and_backward_stay_below_one_matrix_per_triple(torch):
    """B = 4096, K = 5, de = dr = 64, 7 relations: the growth of the peak allocation over forward
    + backward stays below B * de * dr * 4 bytes (67 MB), the size of ONE per-triple matrix block,
    which the composition allocates several times over"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(46)
    b, k, de, dr = 4096, 5, 64, 64
    t = Tabs(torch, gen, de, dr, ent_rows=4096)
    bt = Batch(torch, k, seed=54, b=b, bad=False, ent_rows=4096)
    params = [x.clone().requires_grad_() for x in t.all]
    g_pos, g_neg = upstream(torch, gen, k, "both", b)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    pos, neg = ops.triple_score_matrix(*params, *bt.ids, kind="trans_l1", corrupt="both")
    ((pos * g_pos).sum() + (neg * g_neg).sum()).backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print("\n[triple_score_matrix memory] peak growth %.1f MB, cap %.1f MB" % (growth / 1e6, b * de * dr * 4 / 1e6))
    assert all(p.grad is not None for p in params)
    assert growth < b * de * dr * 4


# ---- E: captured graph, the C entries, the example -------------------------------------------
def test_both_entries_replay_from_a_captured_graph(torch, batches):
    """one stream, a linear chain: forward, then the three kernels of the gradient"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    t = Tabs(torch, gen, 64, 33, "bf16-f32-f16")
    bt = batches[5]
    kind = "trans_l2"
    g_pos, g_neg = upstream(torch, gen, 5, "both")
    order, keys = ops._matrix_grouping(bt.rel_id, REL)
    seg_ptr, seg_rel = ops._matrix_segments(keys, REL, False)
    run_f = lambda: ops._triple_score_matrix_raw(*t.all, *bt.ids, kind, "both", order)   # noqa: E731
    run_g = lambda: ops._triple_score_matrix_grad_raw(*t.all, *bt.ids, kind, "both", order, seg_ptr, seg_rel,   # noqa: E731
                                                      g_pos, g_neg)
    want, want_g = run_f(), run_g()
    assert np_same(want[0], ref.forward(*t.np, *bt.np, kind, "both", t.v)[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_f()                                                                          # (warm up)
        run_g()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = run_f()
            out_g = run_g()
        for _ in range(2):
            for x in out + out_g:
                x.zero_()
            g.replay()
            side.synchronize()
            assert all(same(a, b) for a, b in zip(out + out_g, want + want_g))
    torch.cuda.current_stream().wait_stream(side)


GUARD = -12345.0


class Call(object):
    """euler_gpu_triple_score_matrix / _grad on small buffers with 4 guard words behind every output"""

    def __init__(self, torch):
        from euler_amd import _lib
        self.torch, self.lib = torch, _lib
        self.b, self.k, self.de, self.dr, self.r = 6, 3, 8, 4, 4
        b, k, de, dr = self.b, self.k, self.de, self.dr
        self.ent, self.rel = torch.ones((32, de), device="cuda"), torch.ones((self.r, dr), device="cuda")
        self.matrix = torch.ones((self.r, de * dr), device="cuda")
        self.ids = torch.arange(b, device="cuda")
        self.rel_id = torch.arange(b, device="cuda") % self.r
        self.order = torch.sort(self.rel_id, stable=True)[1].contiguous()
        self.seg_ptr = torch.searchsorted(self.rel_id[self.order], torch.arange(self.r + 1, device="cuda")).contiguous()
        self.seg_rel = torch.arange(self.r, device="cuda")
        self.neg = torch.arange(b * k, device="cuda").reshape(b, k)
        self.g = torch.ones(b * 2 * k, device="cuda")
        self.sizes = dict(pos=b, neg_out=b * 2 * k, g_src=b * de, g_rel=b * dr, g_dst=b * de, g_neg_rows=b * k * de,
                          gz_src=b * dr, gz_dst=b * dr, gz_neg_rows=b * k * dr, g_matrix=self.r * de * dr)
        self.out = {n: torch.full((s + 4,), GUARD, device="cuda") for n, s in self.sizes.items()}

    def p(self, t):
        return C.c_void_p(t.data_ptr())

    def head(self, a):
        return (a["kind"], a["corrupt"], a["ent"], a["ent_dt"], a["ent_rows"], a["de"], a["rel"], a["rel_dt"],
                a["rel_rows"], a["dr"], a["matrix"], a["mat_dt"], a["src"], a["rel_id"], a["dst"], a["neg"], a["b"],
                a["k"], a["order"])

    def base(self):
        base = dict(kind=0, corrupt=2, ent=self.p(self.ent), ent_dt=self.lib.F32, ent_rows=32, de=self.de,
                    rel=self.p(self.rel), rel_dt=self.lib.F32, rel_rows=self.r, dr=self.dr,
                    matrix=self.p(self.matrix), mat_dt=self.lib.F32, src=self.p(self.ids), rel_id=self.p(self.rel_id),
                    dst=self.p(self.ids), neg=self.p(self.neg), b=self.b, k=self.k, order=self.p(self.order),
                    seg_ptr=self.p(self.seg_ptr), seg_rel=self.p(self.seg_rel), nseg=self.r,
                    g_pos=self.p(self.g), g_neg=self.p(self.g))
        base.update({n: self.p(t) for n, t in self.out.items()})
        return base

    def forward(self, **kw):
        from euler_amd.ops import _stream
        a = dict(self.base(), **kw)
        rc = self.lib.lib().euler_gpu_triple_score_matrix(_stream(), *self.head(a), a["pos"], a["neg_out"])
        self.torch.cuda.synchronize()
        return rc

    def grad(self, **kw):
        from euler_amd.ops import _stream
        a = dict(self.base(), **kw)
        rc = self.lib.lib().euler_gpu_triple_score_matrix_grad(
            _stream(), *self.head(a), a["seg_ptr"], a["seg_rel"], a["nseg"], a["g_pos"], a["g_neg"], a["g_src"],
            a["g_rel"], a["g_dst"], a["g_neg_rows"], a["gz_src"], a["gz_dst"], a["gz_neg_rows"], a["g_matrix"])
        self.torch.cuda.synchronize()
        return rc

    def untouched(self, *names):
        return all(bool((self.out[n] == GUARD).all()) for n in (names or self.out))


def test_c_entry_error_rules(torch):
    c = Call(torch)
    EINVAL = c.lib.EINVAL
    for call in (c.forward, c.grad):
        assert call(kind=-1) == EINVAL and call(kind=2) == EINVAL and call(kind=3) == EINVAL   # no distmult
        assert call(corrupt=-1) == EINVAL and call(corrupt=3) == EINVAL
        assert call(ent_dt=3) == EINVAL and call(rel_dt=-1) == EINVAL and call(mat_dt=7) == EINVAL
        assert call(k=-1) == EINVAL and call(de=-1) == EINVAL
        assert call(neg=None) == EINVAL                                   # k > 0 without negatives
        assert call(ent_rows=0) == EINVAL and call(rel_rows=0) == EINVAL and call(ent_rows=1 << 31) == EINVAL
        assert call(b=1 << 30) == EINVAL                                  # b * max(k, 1) * 2 >= 2^31
        assert call(b=1 << 30, k=0) == EINVAL
        assert call(b=1 << 20, k=1 << 10) == EINVAL
        assert call(de=513) == EINVAL and call(dr=513) == EINVAL          # past the cap
        for name in ("ent", "rel", "matrix", "src", "rel_id", "dst", "order"):
            assert call(**{name: None}) == EINVAL, name
    assert c.forward(pos=None) == EINVAL and c.forward(neg_out=None) == EINVAL
    for name in ("g_pos", "g_neg", "g_src", "g_rel", "g_dst", "g_neg_rows", "gz_src", "gz_dst", "gz_neg_rows",
                 "seg_ptr", "seg_rel", "g_matrix"):
        assert c.grad(**{name: None}) == EINVAL, name
    assert c.grad(nseg=-1) == EINVAL and c.grad(nseg=1 << 31) == EINVAL
    assert c.untouched()


def test_c_entry_empty_shapes_guard_words_and_wrong_orders(torch):
    c = Call(torch)
    OK = c.lib.OK
    # b == 0, de == 0 or dr == 0: OK, nothing touched - null buffers included
    for kw in (dict(b=0), dict(de=0), dict(dr=0)):
        assert c.forward(**kw) == OK and c.grad(**kw) == OK
    assert c.forward(b=0, ent=None, matrix=None, src=None, order=None, pos=None) == OK
    assert c.grad(dr=0, g_src=None, g_pos=None, gz_src=None, g_matrix=None) == OK
    assert c.untouched()
    # k == 0: the negative outputs stay untouched (and may be null)
    assert c.forward(k=0) == OK and c.grad(k=0) == OK
    assert c.untouched("neg_out", "g_neg_rows", "gz_neg_rows")
    assert not bool((c.out["pos"][:c.b] == GUARD).any()) and bool((c.out["pos"][c.b:] == GUARD).all())
    assert c.forward(k=0, neg=None, neg_out=None) == OK
    assert c.grad(k=0, neg=None, g_neg=None, g_neg_rows=None, gz_neg_rows=None) == OK
    # nseg == 0: no matrix gradient, the segment arrays may be null
    c1 = Call(torch)
    assert c1.grad(nseg=0, seg_ptr=None, seg_rel=None, g_matrix=None) == OK and c1.untouched("g_matrix")
    # the full call writes exactly its blocks
    for corrupt, kp in ((0, c.k), (1, c.k), (2, 2 * c.k)):
        c2 = Call(torch)
        assert c2.forward(corrupt=corrupt) == OK and c2.grad(corrupt=corrupt) == OK
        sizes = dict(c2.sizes, neg_out=c2.b * kp)
        for n, s in sizes.items():
            assert not bool((c2.out[n][:s] == GUARD).any()) and bool((c2.out[n][s:] == GUARD).all()), (corrupt, n)
    # an order that is no permutation and segment bounds outside [0, b] stay inside the buffers
    c3 = Call(torch)
    wrong = torch.tensor([0, 0, -5, 1 << 40, c3.b, 3], device="cuda")
    far = torch.tensor([-7, 2, 1, 1 << 40, 1 << 41], device="cuda")
    assert c3.forward(order=c3.p(wrong)) == OK and c3.grad(order=c3.p(wrong), seg_ptr=c3.p(far)) == OK
    for n, s in c3.sizes.items():
        assert bool((c3.out[n][s:] == GUARD).all()), n
    assert bool(torch.isfinite(c3.out["g_matrix"]).all())


def test_python_argument_checks(torch):
    from euler_amd import ops
    ent, rel = torch.ones((4, 8), device="cuda"), torch.ones((2, 4), device="cuda")
    mat = torch.ones((2, 32), device="cuda")
    i = torch.zeros(3, dtype=torch.int64, device="cuda")
    for kw in (dict(kind="distmult"), dict(kind="transr"), dict(corrupt="head")):
        with pytest.raises(ValueError):
            ops.triple_score_matrix(ent, rel, mat, i, i, i, **kw)
    for bad in (torch.ones((2, 31), device="cuda"), torch.ones((3, 32), device="cuda"),
                torch.ones((2, 4, 8), device="cuda"), torch.ones(64, device="cuda")):
        with pytest.raises(ValueError):
            ops.triple_score_matrix(ent, rel, bad, i, i, i)
    with pytest.raises(ValueError):
        ops.triple_score_matrix(ent, rel, mat, i, i[:2], i)
    with pytest.raises(ValueError):
        ops.triple_score_matrix(ent, rel, mat, i, i, i, torch.zeros((2, 5), dtype=torch.int64, device="cuda"))
    for tabs in ((ent.double(), rel, mat), (ent, rel.to(torch.int32), mat), (ent, rel, mat.double())):
        with pytest.raises(TypeError):
            ops.triple_score_matrix(*tabs, i, i, i)
    with pytest.raises(RuntimeError):
        ops.triple_score_matrix(ent.cpu(), rel, mat, i, i, i)
    pos = ops.triple_score_matrix(ent, rel, mat.reshape(2, 8, 4), i, i, i)
    assert same(pos, ops.triple_score_matrix(ent, rel, mat, i, i, i))
    empty = ops.triple_score_matrix(ent, rel, mat, i[:0], i[:0], i[:0], i[:0].reshape(0, 5))
    assert empty[0].shape == (0,) and empty[1].shape == (0, 10)
    none = ops.triple_score_matrix(ent[:, :0], rel, mat[:, :0], i, i, i, i.reshape(3, 1))
    assert none[0].shape == (3,) and not bool(none[0].any()) and none[1].shape == (3, 2)
    params = [x.clone().requires_grad_() for x in (ent, rel, mat)]
    out = ops.triple_score_matrix(*params, i[:0], i[:0], i[:0], i[:0].reshape(0, 5))
    (out[0].sum() + out[1].sum()).backward()
    assert all(p.grad.shape == p.shape and not bool(p.grad.any()) for p in params)


@pytest.fixture(scope="module")
def example():
    spec = importlib.util.spec_from_file_location(
        "transr_minibatch", os.path.join(ROOT, "examples", "python", "transr_minibatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("kind", KINDS)
def test_example_step_on_the_fixture_graph(torch, example, kind):
    """one step on the fixture graph, fused against the composition: every score within the
    forward bound of triple_score_matrix_ref (the bound of the host test), a finite loss, and
    SparseAdam moves rows of all three tables"""
    import euler_amd
    G = euler_amd.Graph.load(FIXTURE, edges=True)
    G.set_seed(7)
    batch, negs, de, dr = 64, 5, 32, 24
    n_ent, n_rel = G.id_range()[0] + 1, G.num_edge_types
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    start = example.make_tables(n_ent, n_rel, de, dr, gen=gen)
    src, rel_id, dst, neg = example.sample_batch(G, batch, negs)
    scores, losses, rows = {}, {}, {}
    for composed in (False, True):
        tables = {name: torch.nn.Parameter(t.detach().clone()) for name, t in start.items()}
        opt = torch.optim.SparseAdam(list(tables.values()), lr=0.01)
        pos, out = example.energies(tables, src, rel_id, dst, neg, kind, composed)
        loss = example.margin_loss(pos, out)
        opt.zero_grad()
        loss.backward()
        opt.step()
        scores[composed], losses[composed] = (pos.detach(), out.detach()), float(loss.detach())
        rows[composed] = [int((tables[n].detach() != start[n].detach()).any(1).sum()) for n in ("ent", "rel", "matrix")]
    ids = [t.cpu().numpy() for t in (src, rel_id, dst, neg)]
    tabs = [start[n].detach().float().cpu().numpy() for n in ("ent", "rel", "matrix")]
    _, _, mag_pos, mag_neg = ref.forward64(*tabs, *ids, kind, "both")
    worst = 0.0
    for fused, comp, mag in zip(scores[False], scores[True], (mag_pos, mag_neg)):
        diff = (fused.double() - comp.double()).abs().cpu().numpy()
        bound = ref.forward_bound(kind, de, dr, mag)
        assert np.all(diff <= bound), (kind, float((diff / bound).max()))
        worst = max(worst, float((diff / bound).max()))
    print("\n[transr %s example] fused loss %.9g composed %.9g, worst |score diff| / bound = %.4f"
          % (kind, losses[False], losses[True], worst))
    assert np.isfinite(losses[False]) and np.isfinite(losses[True])
    assert all(r > 0 for r in rows[False]) and all(r > 0 for r in rows[True])


@pytest.mark.parametrize("mode", [[], ["--kind", "trans_l2"], ["--composed"]])
def test_example_runs(mode):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", "transr_minibatch.py")] + mode,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "loss" in r.stdout and "matrices" in r.stdout and ("composed" in r.stdout) == ("--composed" in mode), \
        r.stdout
