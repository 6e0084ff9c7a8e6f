"""Triple scoring with the TransH / TransD projections on the GPU (ops.triple_score_proj,
euler_gpu_triple_score_proj[_grad]):
  A  forward bits == the numpy restatement tests/triple_score_proj_ref.py (dtypes, d, unaligned
     views, the grid stride)
  B  per-occurrence gradient bits == the restatement; the tables' gradients == ops.scatter_add of
     those rows in occurrence order; sparse_grad; repeated and out-of-range ids
  C  both entries replay from a captured graph
  D  the rules of the C entries; empty shapes; guard words; the Python argument checks
  E  the example's step on the fixture graph, fused against --composed"""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_half_mp_gpu import DIMS, same
import triple_score_proj_ref as ref

pytestmark = pytest.mark.gpu

ENT, REL, B = 300, 7, 90
PROJS, KINDS, CORRUPTS = ("hyperplane", "transfer"), ("trans_l1", "trans_l2"), ("front", "tail", "both")
FIXTURE = os.path.join(ROOT, "tests", "golden", "fixture_dat")
NAMES = ("src", "rel", "dst", "neg", "rel_aux", "src_aux", "dst_aux", "neg_aux")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def pairs(torch):
    f, b, h = torch.float32, torch.bfloat16, torch.float16
    return {"f32": (f, f), "bf16": (b, b), "f16": (h, h), "bf16-f32": (b, f), "f32-f16": (f, h)}


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
    """the five tables in the storage pair S; of(proj) -> (ent, ent_aux | None, rel, rel_aux)"""

    def __init__(self, torch, gen, d, S, unaligned=(), ent_rows=ENT, rel_rows=REL):
        SE, SR = pairs(torch)[S] if isinstance(S, str) else S
        mk = lambda name, rows, dt, scale: draw(torch, gen, (rows, d), dt, name in unaligned, scale)   # noqa: E731
        self.ent, self.ent_transfer = mk("ent", ent_rows, SE, 4.0), mk("ent_transfer", ent_rows, SE, 1.0)
        self.rel, self.hyper = mk("rel", rel_rows, SR, 4.0), mk("hyper", rel_rows, SR, 4.0)
        self.rel_transfer = mk("rel_transfer", rel_rows, SR, 1.0)

    def of(self, proj):
        if proj == "hyperplane":
            return self.ent, None, self.rel, self.hyper
        return self.ent, self.ent_transfer, self.rel, self.rel_transfer

    def kw(self, proj):
        if proj == "hyperplane":
            return dict(proj=proj, hyper=self.hyper)
        return dict(proj=proj, ent_transfer=self.ent_transfer, rel_transfer=self.rel_transfer)


class Batch(object):
    """B triples with K negatives over ENT / REL rows: ids repeat inside the batch, a negative
    equals its src, and some ids name no row (-1, rows + 3, 2^33 + 5)"""

    def __init__(self, torch, k, seed=3, b=B, bad=True, ent_rows=ENT, rel_rows=REL):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed + k)
        r = lambda hi, shape: torch.randint(0, hi, shape, generator=gen, device="cuda")      # noqa: E731
        self.k = k
        self.src, self.dst, self.rel_id = r(ent_rows, (b,)), r(ent_rows, (b,)), r(rel_rows, (b,))
        self.neg = r(ent_rows, (b, k)) if k else None
        self.src[5] = self.src[4]
        self.dst[6] = self.src[4]
        if bad:
            self.src[10], self.dst[11], self.rel_id[12] = -1, ent_rows + 3, (1 << 33) + 5
            self.src[13], self.rel_id[14] = (1 << 33) + 5, -1
        if k:
            self.neg[4, 0] = self.src[4]
            self.neg[7, k - 1] = self.dst[6]
            if bad:
                self.neg[15, 0], self.neg[16, k - 1] = -1, ent_rows + 3
        self.np = [None if t is None else t.cpu().numpy() for t in (self.src, self.rel_id, self.dst, self.neg)]
        self.ids = (self.src, self.rel_id, self.dst, self.neg)

    def ent_keys(self):
        return np.concatenate([self.np[0], self.np[2]] + ([self.np[3].reshape(-1)] if self.k else []))


@pytest.fixture(scope="module")
def batches(torch):
    return {k: Batch(torch, k) for k in (0, 1, 5)}


def widened(t):
    return None if t is None else t.float().cpu().numpy()


def width(tabs):
    ent, ent_aux, rel, rel_aux = tabs
    return ref.proj_chunk_width(ent.shape[1], ent.data_ptr(), 0 if ent_aux is None else ent_aux.data_ptr(),
                                ent.element_size(), rel.data_ptr(), rel_aux.data_ptr(), rel.element_size())


def np_same(got, want):
    if got is None or want is None:
        return got is None and want is None
    got = got.cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


def upstream(torch, gen, k, corrupt, b=B):
    kp = 2 * k if corrupt == "both" else k
    return draw(torch, gen, (b,), torch.float32), (draw(torch, gen, (b, kp), torch.float32) if k else None)


def configs(d, full):
    """(proj, kind, corrupt, K): the full cross, or per d both projections with the rest rotating"""
    if full:
        return [(p, kind, c, k) for p in PROJS for kind in KINDS for k in (0, 1, 5)
                for c in (CORRUPTS if k else ("both",))]
    i = DIMS.index(d)
    return [(p, KINDS[(i + j + q) % 2], CORRUPTS[(i + j) % 3] if k else "both", k)
            for q, p in enumerate(PROJS) for j, k in enumerate((0, 1, 5))]


def fwd(ops, t, proj, bt, kind, corrupt):
    return ops.triple_score_proj(t.ent, t.rel, *bt.ids, kind=kind, corrupt=corrupt, **t.kw(proj))


def want_fwd(t, proj, bt_np, kind, corrupt, v):
    return ref.forward(proj, *[widened(x) for x in t.of(proj)], *bt_np, kind, corrupt, v)


def want_grad(t, proj, bt_np, kind, corrupt, v, g_pos, g_neg):
    return ref.grad(proj, *[widened(x) for x in t.of(proj)], *bt_np, kind, corrupt, v, widened(g_pos),
                    widened(g_neg))


# ---- A: forward bits -------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("S", ["f32", "bf16", "f16", "bf16-f32", "f32-f16"])
def test_forward_has_the_bits_of_the_restatement(torch, batches, S, d):
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(100 + d)
    t = Tabs(torch, gen, d, S)
    for proj, kind, corrupt, k in configs(d, d in (1, 20, 520)):
        v = width(t.of(proj))
        assert v == (8 if d % 8 == 0 else 4 if d % 4 == 0 else 1)
        bt = batches[k]
        got = fwd(ops, t, proj, bt, kind, corrupt)
        want_pos, want_neg = want_fwd(t, proj, bt.np, kind, corrupt, v)
        tag = (proj, kind, corrupt, k)
        if k == 0:
            assert torch.is_tensor(got) and np_same(got, want_pos), tag
        else:
            assert np_same(got[0], want_pos) and np_same(got[1], want_neg), tag
            assert got[1].shape == (B, 2 * k if corrupt == "both" else k)


@pytest.mark.parametrize("d", [8, 64, 520])
@pytest.mark.parametrize("S", ["f32", "bf16", "bf16-f32"])
def test_forward_and_gradient_on_unaligned_views(torch, batches, S, d):
    """tables that start one element into their storage: V = 1; one such table among aligned
    ones is enough - the rule looks at every table passed"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(200 + d)
    every = ("ent", "ent_transfer", "rel", "hyper", "rel_transfer")
    bt = batches[5]
    for j, (proj, off) in enumerate((("hyperplane", every), ("transfer", every), ("hyperplane", ("hyper",)),
                                     ("transfer", ("ent_transfer",)), ("transfer", ("rel_transfer",)))):
        t = Tabs(torch, gen, d, S, unaligned=off)
        tabs = t.of(proj)
        assert width(tabs) == 1
        kind = KINDS[j % 2]
        pos, neg = fwd(ops, t, proj, bt, kind, "both")
        want = want_fwd(t, proj, bt.np, kind, "both", 1)
        assert np_same(pos, want[0]) and np_same(neg, want[1]), (proj, off)
        g_pos, g_neg = upstream(torch, gen, 5, "both")
        got = ops._triple_score_proj_grad_raw(proj, *tabs, *bt.ids, kind, "both", g_pos, g_neg)
        want = want_grad(t, proj, bt.np, kind, "both", 1, g_pos, g_neg)
        assert all(np_same(g, w) for g, w in zip(got, want)), (proj, off)


@pytest.mark.parametrize("proj", PROJS)
def test_grid_stride(torch, proj):
    """d = 1 gives 64 triples a wave and the launcher caps the grid at 32768 waves: with
    B = 64 * 32768 + 300 the last 300 triples are a wave's second task.  Triples are independent:
    the restatement is taken for the first 64 and the last 364, the rest is held against a
    second call."""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    d, b = 1, 64 * 32768 + 300
    sel = np.concatenate([np.arange(64), np.arange(b - 364, b)])
    pick = lambda ids: [None if x is None else x[sel] for x in ids]                      # noqa: E731
    t = Tabs(torch, gen, d, "f32")
    bt = Batch(torch, 0, seed=40, b=b)
    pos = fwd(ops, t, proj, bt, "trans_l1", "both")
    want = want_fwd(t, proj, pick(bt.np), "trans_l1", "both", 1)
    assert pos.shape == (b,) and np_same(pos[sel], want[0])
    assert same(pos, fwd(ops, t, proj, bt, "trans_l1", "both"))
    g_pos = draw(torch, gen, (b,), torch.float32)
    got = ops._triple_score_proj_grad_raw(proj, *t.of(proj), *bt.ids, "trans_l1", "both", g_pos, None)
    again = ops._triple_score_proj_grad_raw(proj, *t.of(proj), *bt.ids, "trans_l1", "both", g_pos, None)
    want = want_grad(t, proj, pick(bt.np), "trans_l1", "both", 1, g_pos[sel], None)
    for g, g2, w, name in zip(got, again, want, NAMES):
        if name in ("neg", "neg_aux"):
            assert g is None or g.shape == (b, 0, d)
        else:
            assert (g is None and w is None) or (np_same(g[sel], w) and same(g, g2)), name


# ---- B: gradient bits ------------------------------------------------------------------------
def scattered(torch, ops, rows, keys, n_rows, dt):
    keys = np.where((keys >= 0) & (keys < n_rows), keys, -1).astype(np.int32)
    return ops.scatter_add(torch.from_numpy(rows).cuda(), torch.from_numpy(keys).cuda(), n_rows).to(dt)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("S", ["f32", "bf16", "f32-f16"])
def test_gradients_have_the_bits_of_the_restatement(torch, batches, S, d):
    """the kernel's rows == the restatement's; the gradient of every table == ops.scatter_add of
    the restatement's rows at [src | dst | neg] / rel_id (ids that name no row: key -1), rounded
    once.  Every (proj, kind, K) at every d with corrupt rotating; all three corrupt modes at
    d = 3, 20 (the register form) and d = 64, 520 (the memory form)."""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(300 + d)
    t = Tabs(torch, gen, d, S)
    i = DIMS.index(d)
    combos = [(p, kind, k) for p in PROJS for kind in KINDS for k in (0, 1, 5)]
    for j, (proj, kind, k) in enumerate(combos):
        tabs = t.of(proj)
        v = width(tabs)
        bt = batches[k]
        for corrupt in (CORRUPTS if k and d in (3, 20, 64, 520) else (CORRUPTS[(i + j) % 3] if k else "both",)):
            g_pos, g_neg = upstream(torch, gen, k, corrupt)
            tag = (proj, kind, corrupt, k)
            got = ops._triple_score_proj_grad_raw(proj, *tabs, *bt.ids, kind, corrupt, g_pos, g_neg)
            want = want_grad(t, proj, bt.np, kind, corrupt, v, g_pos, g_neg)
            for g, w, name in zip(got, want, NAMES):
                assert np_same(g, w), tag + (name,)
        if j != i % len(combos) and j != (i + 7) % len(combos):
            continue                                          # the autograd path: two configurations per d
        params = [None if x is None else x.clone().requires_grad_() for x in tabs]
        kw = dict(proj=proj, hyper=params[3]) if proj == "hyperplane" else \
            dict(proj=proj, ent_transfer=params[1], rel_transfer=params[3])
        out = ops.triple_score_proj(params[0], params[2], *bt.ids, kind=kind, corrupt=corrupt, **kw)
        loss = (out * g_pos).sum() if k == 0 else (out[0] * g_pos).sum() + (out[1] * g_neg).sum()
        loss.backward()
        ent_rows = lambda a, c, n: np.concatenate([a, c] + ([n.reshape(-1, d)] if k else []))   # noqa: E731
        assert same(params[0].grad, scattered(torch, ops, ent_rows(want[0], want[2], want[3]), bt.ent_keys(), ENT,
                                              tabs[0].dtype)), tag
        assert same(params[2].grad, scattered(torch, ops, want[1], bt.np[1], REL, tabs[2].dtype)), tag
        assert same(params[3].grad, scattered(torch, ops, want[4], bt.np[1], REL, tabs[3].dtype)), tag
        if proj == "transfer":
            assert same(params[1].grad, scattered(torch, ops, ent_rows(want[5], want[6], want[7]), bt.ent_keys(), ENT,
                                                  tabs[1].dtype)), tag
        assert all(p is None or p.grad.dtype == p.dtype for p in params)


@pytest.mark.parametrize("S", ["f32", "bf16"])
@pytest.mark.parametrize("proj", PROJS)
def test_sparse_grad_equals_the_dense_gradient_on_its_rows(torch, batches, S, proj):
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    t = Tabs(torch, gen, 20, S)
    bt = batches[5]
    g_pos, g_neg = upstream(torch, gen, 5, "both")
    grads = {}
    for sparse in (False, True):
        params = [None if x is None else x.clone().requires_grad_() for x in t.of(proj)]
        kw = dict(proj=proj, hyper=params[3]) if proj == "hyperplane" else \
            dict(proj=proj, ent_transfer=params[1], rel_transfer=params[3])
        pos, neg = ops.triple_score_proj(params[0], params[2], *bt.ids, kind="trans_l2", sparse_grad=sparse, **kw)
        ((pos * g_pos).sum() + (neg * g_neg).sum()).backward()
        grads[sparse] = [None if p is None else p.grad for p in params]
    for dense, sp, keys, rows in zip(grads[False], grads[True], (bt.ent_keys(), bt.ent_keys(), bt.np[1], bt.np[1]),
                                     (ENT, ENT, REL, REL)):
        if dense is None:
            assert sp is None
            continue
        assert sp.is_sparse and sp.shape == dense.shape and sp.dtype == dense.dtype
        sp = sp.coalesce()
        idx = sp.indices()[0]
        looked_up = np.unique(keys[(keys >= 0) & (keys < rows)])
        assert np.array_equal(idx.cpu().numpy(), looked_up)               # absent elsewhere
        assert same(sp.values(), dense[idx])
        rest = torch.ones(rows, dtype=torch.bool, device="cuda")
        rest[idx] = False
        assert not bool(dense[rest].any())


@pytest.mark.parametrize("proj", PROJS)
def test_repeated_ids_accumulate_and_bad_ids_get_nothing(torch, batches, proj):
    """triples 4, 5, 6 share src[4] as src, src, dst, and negative (4, 0) is src[4] too"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    d = 64
    t = Tabs(torch, gen, d, "f32")
    tabs = t.of(proj)
    bt = batches[5]
    g_pos, g_neg = upstream(torch, gen, 5, "both")
    gs, gr, gd, gn, gra, gsa, gda, gna = ops._triple_score_proj_grad_raw(proj, *tabs, *bt.ids, "trans_l1", "both",
                                                                         g_pos, g_neg)
    every = torch.ones(B, dtype=torch.bool, device="cuda")
    blocks = [(gs, bt.src, ENT, every), (gd, bt.dst, ENT, every), (gr, bt.rel_id, REL, every),
              (gn, bt.neg, ENT, every), (gra, bt.rel_id, REL, every)]
    if proj == "transfer":
        # ga = (gz . rho) x: a triple whose rel_id names no row has rho = 0 and passes ent_transfer nothing
        has_rho = (bt.rel_id >= 0) & (bt.rel_id < REL)
        blocks += [(gsa, bt.src, ENT, has_rho), (gda, bt.dst, ENT, has_rho), (gna, bt.neg, ENT, has_rho)]
    for rows, ids, n_rows, expect in blocks:
        off = (ids < 0) | (ids >= n_rows)
        expect = expect if ids.dim() == 1 else expect.unsqueeze(1).expand_as(ids)
        assert int(off.sum()) >= 1 and not bool(rows[off].any()) and bool(rows[~off & expect].any(-1).all())
        assert not bool(rows[~expect].any())
    params = [None if x is None else x.clone().requires_grad_() for x in tabs]
    kw = dict(proj=proj, hyper=params[3]) if proj == "hyperplane" else \
        dict(proj=proj, ent_transfer=params[1], rel_transfer=params[3])
    pos, neg = ops.triple_score_proj(params[0], params[2], *bt.ids, kind="trans_l1", **kw)
    ((pos * g_pos).sum() + (neg * g_neg).sum()).backward()
    node = int(bt.src[4])
    keys = torch.from_numpy(bt.ent_keys()).cuda()
    at = (keys == node).nonzero().reshape(-1)
    assert at.numel() >= 4
    for param, (a, c, n) in ((params[0], (gs, gd, gn)), (params[1], (gsa, gda, gna))):
        if param is None:
            continue
        rows = torch.cat([a, c, n.reshape(-1, d)])
        acc = torch.zeros(d, device="cuda")
        for p in at.tolist():                                 # the occurrence order [src | dst | neg]
            acc = acc + rows[p]
        assert same(param.grad[node], acc)


# ---- C: captured graph -----------------------------------------------------------------------
@pytest.mark.parametrize("proj", PROJS)
def test_both_entries_replay_from_a_captured_graph(torch, batches, proj):
    """one stream, a linear chain: forward then gradient"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(31)
    t = Tabs(torch, gen, 128, "bf16-f32")
    tabs = t.of(proj)
    bt = batches[5]
    kind = "trans_l2"
    g_pos, g_neg = upstream(torch, gen, 5, "both")
    live = lambda xs: tuple(x for x in xs if x is not None)                              # noqa: E731
    want = fwd(ops, t, proj, bt, kind, "both")
    want_g = live(ops._triple_score_proj_grad_raw(proj, *tabs, *bt.ids, kind, "both", g_pos, g_neg))
    assert np_same(want[0], want_fwd(t, proj, bt.np, kind, "both", width(tabs))[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd(ops, t, proj, bt, kind, "both")                                              # (warm up)
        ops._triple_score_proj_grad_raw(proj, *tabs, *bt.ids, kind, "both", g_pos, g_neg)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = fwd(ops, t, proj, bt, kind, "both")
            out_g = live(ops._triple_score_proj_grad_raw(proj, *tabs, *bt.ids, kind, "both", g_pos, g_neg))
        for _ in range(2):
            for x in out + out_g:
                x.zero_()
            g.replay()
            side.synchronize()
            assert all(same(a, b) for a, b in zip(out + out_g, want + want_g))
    torch.cuda.current_stream().wait_stream(side)


# ---- D: the C entries ------------------------------------------------------------------------
GUARD = -12345.0


class Call(object):
    """euler_gpu_triple_score_proj / _grad on small buffers with 4 guard words behind every output"""

    def __init__(self, torch, proj):
        from euler_amd import _lib
        self.torch, self.lib, self.proj = torch, _lib, proj
        self.b, self.k, self.d = 6, 3, 8
        b, k, d = self.b, self.k, self.d
        self.ent, self.ent_aux = torch.ones((32, d), device="cuda"), torch.ones((32, d), device="cuda")
        self.rel, self.rel_aux = torch.ones((4, d), device="cuda"), torch.ones((4, d), device="cuda")
        self.ids = torch.arange(b, device="cuda")
        self.neg = torch.arange(b * k, device="cuda").reshape(b, k)
        self.g = torch.ones(b * 2 * k, device="cuda")
        self.sizes = dict(pos=b, neg_out=b * 2 * k, g_src=b * d, g_rel=b * d, g_dst=b * d, g_neg_rows=b * k * d,
                          g_rel_aux=b * d)
        if proj == 2:
            self.sizes.update(g_src_aux=b * d, g_dst_aux=b * d, g_neg_aux_rows=b * k * d)
        self.out = {n: torch.full((s + 4,), GUARD, device="cuda") for n, s in self.sizes.items()}

    def p(self, t):
        return C.c_void_p(t.data_ptr())

    def head(self, a):
        return (a["proj"], a["kind"], a["corrupt"], a["ent"], a["ent_aux"], a["ent_dt"], a["ent_rows"], a["rel"],
                a["rel_aux"], a["rel_dt"], a["rel_rows"], a["src"], a["rel_id"], a["dst"], a["neg"], a["b"], a["k"],
                a["d"])

    def base(self):
        base = dict(proj=self.proj, kind=0, corrupt=2, ent=self.p(self.ent),
                    ent_aux=self.p(self.ent_aux) if self.proj == 2 else None, ent_dt=self.lib.F32, ent_rows=32,
                    rel=self.p(self.rel), rel_aux=self.p(self.rel_aux), rel_dt=self.lib.F32, rel_rows=4,
                    src=self.p(self.ids), rel_id=self.p(self.ids), dst=self.p(self.ids), neg=self.p(self.neg),
                    b=self.b, k=self.k, d=self.d, g_pos=self.p(self.g), g_neg=self.p(self.g),
                    g_src_aux=None, g_dst_aux=None, g_neg_aux_rows=None)
        base.update({n: self.p(t) for n, t in self.out.items()})
        return base

    def forward(self, **kw):
        from euler_amd.ops import _stream
        a = dict(self.base(), **kw)
        rc = self.lib.lib().euler_gpu_triple_score_proj(_stream(), *self.head(a), a["pos"], a["neg_out"])
        self.torch.cuda.synchronize()
        return rc

    def grad(self, **kw):
        from euler_amd.ops import _stream
        a = dict(self.base(), **kw)
        rc = self.lib.lib().euler_gpu_triple_score_proj_grad(
            _stream(), *self.head(a), a["g_pos"], a["g_neg"], a["g_src"], a["g_rel"], a["g_dst"], a["g_neg_rows"],
            a["g_rel_aux"], a["g_src_aux"], a["g_dst_aux"], a["g_neg_aux_rows"])
        self.torch.cuda.synchronize()
        return rc

    def untouched(self, *names):
        return all(bool((self.out[n] == GUARD).all()) for n in (names or self.out))


@pytest.mark.parametrize("proj", [1, 2])
def test_c_entry_error_rules(torch, proj):
    c = Call(torch, proj)
    EINVAL = c.lib.EINVAL
    spare = c.p(torch.ones((32, 8), device="cuda"))
    for call in (c.forward, c.grad):
        assert call(proj=0) == EINVAL and call(proj=3) == EINVAL
        assert call(kind=-1) == EINVAL and call(kind=2) == EINVAL and call(kind=3) == EINVAL   # no distmult
        assert call(corrupt=-1) == EINVAL and call(corrupt=3) == EINVAL
        assert call(ent_dt=3) == EINVAL and call(rel_dt=-1) == EINVAL
        assert call(k=-1) == EINVAL
        assert call(neg=None) == EINVAL                                   # k > 0 without negatives
        assert call(ent_rows=0) == EINVAL and call(rel_rows=0) == EINVAL
        assert call(b=1 << 30) == EINVAL                                  # b * max(k, 1) * 2 >= 2^31
        assert call(b=1 << 30, k=0) == EINVAL
        assert call(b=1 << 20, k=1 << 10) == EINVAL
        assert call(d=1 << 31) == EINVAL
        for name in ("ent", "rel", "src", "rel_id", "dst", "rel_aux"):
            assert call(**{name: None}) == EINVAL, name
        if proj == 1:
            assert call(ent_aux=spare) == EINVAL                          # an aux table that should be NULL
        else:
            assert call(ent_aux=None) == EINVAL                           # a missing aux table
    assert c.forward(pos=None) == EINVAL and c.forward(neg_out=None) == EINVAL
    for name in ("g_pos", "g_neg", "g_src", "g_rel", "g_dst", "g_neg_rows", "g_rel_aux"):
        assert c.grad(**{name: None}) == EINVAL, name
    for name in ("g_src_aux", "g_dst_aux", "g_neg_aux_rows"):
        assert c.grad(**{name: spare if proj == 1 else None}) == EINVAL, name
    assert c.untouched()


@pytest.mark.parametrize("proj", [1, 2])
def test_c_entry_empty_shapes_and_guard_words(torch, proj):
    c = Call(torch, proj)
    OK = c.lib.OK
    # b == 0 or d == 0: OK, nothing touched - null buffers included
    assert c.forward(b=0) == OK and c.grad(b=0) == OK and c.forward(d=0) == OK and c.grad(d=0) == OK
    assert c.forward(b=0, ent=None, rel_aux=None, src=None, pos=None) == OK
    assert c.grad(d=0, g_src=None, g_pos=None, g_rel_aux=None) == OK
    assert c.untouched()
    # k == 0: the negative outputs stay untouched (and may be null)
    assert c.forward(k=0) == OK and c.grad(k=0) == OK
    assert c.untouched("neg_out", "g_neg_rows", *(("g_neg_aux_rows",) if proj == 2 else ()))
    assert not bool((c.out["pos"][:c.b] == GUARD).any()) and bool((c.out["pos"][c.b:] == GUARD).all())
    assert c.forward(k=0, neg=None, neg_out=None) == OK
    assert c.grad(k=0, neg=None, g_neg=None, g_neg_rows=None, g_neg_aux_rows=None) == OK
    # the full call writes exactly [B] / [B, K'] / [B, d] / [B, K, d]
    for corrupt, kp in ((0, c.k), (1, c.k), (2, 2 * c.k)):
        c2 = Call(torch, proj)
        assert c2.forward(corrupt=corrupt) == OK and c2.grad(corrupt=corrupt) == OK
        sizes = dict(c2.sizes, neg_out=c2.b * kp)
        for n, s in sizes.items():
            assert not bool((c2.out[n][:s] == GUARD).any()) and bool((c2.out[n][s:] == GUARD).all()), (corrupt, n)


def test_python_argument_checks(torch):
    from euler_amd import ops
    ent, rel = torch.ones((4, 8), device="cuda"), torch.ones((2, 8), device="cuda")
    i = torch.zeros(3, dtype=torch.int64, device="cuda")
    H = dict(proj="hyperplane", hyper=rel)
    D = dict(proj="transfer", ent_transfer=ent, rel_transfer=rel)
    for kw in (dict(H, proj="transr"), dict(H, kind="distmult"), dict(D, kind="transh"), dict(H, corrupt="head"),
               dict(proj="hyperplane"), dict(H, ent_transfer=ent), dict(H, rel_transfer=rel),
               dict(D, hyper=rel), dict(proj="transfer", ent_transfer=ent), dict(proj="transfer", rel_transfer=rel),
               dict(H, hyper=rel[:1]), dict(D, ent_transfer=ent[:2]),
               dict(D, rel_transfer=torch.ones((2, 4), device="cuda"))):
        with pytest.raises(ValueError):
            ops.triple_score_proj(ent, rel, i, i, i, **kw)
    with pytest.raises(ValueError):
        ops.triple_score_proj(ent, torch.ones((2, 4), device="cuda"), i, i, i, **H)
    with pytest.raises(ValueError):
        ops.triple_score_proj(ent, rel, i, i[:2], i, **H)
    with pytest.raises(TypeError):
        ops.triple_score_proj(ent.double(), rel, i, i, i, **H)
    with pytest.raises(TypeError):
        ops.triple_score_proj(ent, rel, i, i, i, proj="hyperplane", hyper=rel.half())
    with pytest.raises(TypeError):
        ops.triple_score_proj(ent, rel, i, i, i, **dict(D, ent_transfer=ent.bfloat16()))
    with pytest.raises(RuntimeError):
        ops.triple_score_proj(ent.cpu(), rel, i, i, i, **H)
    for kw in (H, D):
        empty = ops.triple_score_proj(ent, rel, i[:0], i[:0], i[:0], i[:0].reshape(0, 5), **kw)
        assert empty[0].shape == (0,) and empty[1].shape == (0, 10)
    none = ops.triple_score_proj(ent[:, :0], rel[:, :0], i, i, i, i.reshape(3, 1), proj="hyperplane", hyper=rel[:, :0])
    assert none[0].shape == (3,) and not bool(none[0].any()) and none[1].shape == (3, 2)


# ---- E: the example's step -------------------------------------------------------------------
@pytest.fixture(scope="module")
def example():
    spec = importlib.util.spec_from_file_location(
        "transh_transd_minibatch", os.path.join(ROOT, "examples", "python", "transh_transd_minibatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("proj", PROJS)
@pytest.mark.parametrize("kind", KINDS)
def test_example_step_on_the_fixture_graph(torch, example, proj, kind):
    """one step on the fixture graph, fused against the composition: every score within the
    forward bound of triple_score_proj_ref, a finite loss, and SparseAdam moves rows"""
    import euler_amd
    G = euler_amd.Graph.load(FIXTURE, edges=True)
    G.set_seed(7)
    batch, negs, d = 64, 5, 32
    n_ent, n_rel = G.id_range()[0] + 1, G.num_edge_types
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    start = example.make_tables(proj, n_ent, n_rel, d, gen=gen)
    src, rel_id, dst, neg = example.sample_batch(G, batch, negs)
    scores, losses, rows = {}, {}, {}
    for composed in (False, True):
        tables = {name: torch.nn.Parameter(t.detach().clone()) for name, t in start.items()}
        opt = torch.optim.SparseAdam(list(tables.values()), lr=0.01)
        pos, out = example.energies(proj, tables, src, rel_id, dst, neg, kind, composed)
        loss = example.margin_loss(pos, out)
        opt.zero_grad()
        loss.backward()
        opt.step()
        scores[composed], losses[composed] = (pos.detach(), out.detach()), float(loss.detach())
        rows[composed] = int((tables["ent"].detach() != start["ent"].detach()).any(1).sum())
    ids = [t.cpu().numpy() for t in (src, rel_id, dst, neg)]
    aux = ("hyper",) if proj == "hyperplane" else ("ent_transfer", "rel_transfer")
    tabs = [widened(start["ent"].detach()), widened(start["ent_transfer"].detach()) if proj == "transfer" else None,
            widened(start["rel"].detach()), widened(start[aux[-1]].detach())]
    _, _, mag_pos, mag_neg = ref.forward64(proj, *tabs, *ids, kind, "both")
    worst = 0.0
    for fused, comp, mag in zip(scores[False], scores[True], (mag_pos, mag_neg)):
        diff = (fused.double() - comp.double()).abs().cpu().numpy()
        bound = ref.forward_bound(proj, kind, d, mag)
        assert np.all(diff <= bound), (proj, kind, float((diff / bound).max()))
        worst = max(worst, float((diff / bound).max()))
    print("\n[%s %s example] fused loss %.9g composed %.9g, worst |score diff| / bound = %.4f"
          % (proj, kind, losses[False], losses[True], worst))
    assert np.isfinite(losses[False]) and np.isfinite(losses[True])
    assert rows[False] > 0 and rows[True] > 0


@pytest.mark.parametrize("mode", [["--proj", "hyperplane"], ["--proj", "transfer", "--kind", "trans_l2"],
                                  ["--proj", "transfer", "--composed"]])
def test_example_runs(mode):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", "transh_transd_minibatch.py")] + mode,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "loss" in r.stdout and "rows updated" in r.stdout and ("composed" in r.stdout) == ("--composed" in mode), \
        r.stdout
