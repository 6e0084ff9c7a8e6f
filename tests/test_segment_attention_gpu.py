"""ops.attention_aggregate on the GPU.
A. Bits against the numpy restatement tests/segment_attention_ref.py (fp32: out, alpha, the
   destination-side gradient) through seg_ptr, sorted keys and unsorted keys; two calls agree.
B. Bits against the existing ops: alpha is edge_softmax of the op's own logits, out the weighted
   gather_segment_reduce with alpha, the three gradients the compositions built from edge_softmax's
   backward and gather_scatter.
C. bf16 / fp16 tables give the bits of the fp32 op on the widened inputs; a 16-bit out_dtype those
   bits after one .to().
D. The forward against float64 within the bound derived in DESIGN 4.20, unpadded.
E. v=None equals v=k.  F. Empty destinations: zero rows, zero gradients.  G. Argument errors.
The gradients are also run through unsorted keys with keys outside [0, size), with Dv != D, with int64
ids and with 16-bit tables."""
import numpy as np
import pytest
import torch

import segment_attention_ref as ref

pytestmark = pytest.mark.gpu

ROWS = 300
# (heads, D): the short kernel's vector and element chunks, several heads a group, head counts that
# do not divide 64, and two shapes only the block-per-destination kernel serves (1, 512), (8, 1024)
SHAPES = [(1, 1), (1, 4), (4, 4), (1, 20), (4, 20), (3, 15), (3, 96), (1, 128), (4, 128), (8, 128)]
LONG_ONLY = [(1, 512), (8, 1024)]
MIXED = [0, 1, 32, 33, 300, 1025, 10, 0, 17]


def dev(a):
    return None if a is None else torch.as_tensor(a, device="cuda")


def bits(t):
    return t.detach().cpu().contiguous().view(-1).view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a) == bits(b)).all())


def same_np(t, a):
    got = t.detach().cpu().numpy()
    return got.dtype == a.dtype == np.float32 and got.shape == a.shape and \
        np.array_equal(got.view(np.uint32), a.view(np.uint32))


class Block(object):
    """the numpy side of one call: tables of `rows` rows, gather rows, destinations by seg_ptr"""

    def __init__(self, kind, heads, d, lens, shared=False, rows=ROWS, q_index=False, with_q=True, seed=0,
                 dv=None, scale=0.37, slope=0.2):
        rng = np.random.default_rng(seed + 131 * heads + d)
        self.kind, self.heads, self.scale, self.slope = kind, heads, scale, slope
        lens = np.asarray(lens, np.int64)
        self.sp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.size, self.e = len(lens), int(self.sp[-1])
        dk = heads if kind == "additive" else d
        self.dv = dk if shared else (dv or d)
        q_rows = 7 if q_index else max(self.size, 1)
        self.q = (rng.standard_normal((q_rows, dk)) * 0.7).astype(np.float32) if with_q else None
        self.qi = rng.integers(0, 7, self.size).astype(np.int32) if q_index and with_q else None
        self.k = (rng.standard_normal((rows, dk)) * 0.7).astype(np.float32)
        self.v = None if shared else rng.standard_normal((rows, self.dv)).astype(np.float32)
        self.gi = rng.integers(0, rows, self.e).astype(np.int32)
        self.grad = rng.standard_normal((self.size, self.dv)).astype(np.float32)
        self.keys = np.repeat(np.arange(self.size, dtype=np.int32), lens)

    def want(self):
        return ref.forward(self.kind, self.q, self.k, self.v, self.gi, self.sp, self.heads, q_index=self.qi,
                           scale=self.scale, slope=self.slope)

    def call(self, ops, q=None, k=None, v=None, gi=None, **kw):
        """through ops; the segment form in kw (default seg_ptr)"""
        if not any(n in kw for n in ("indices", "seg_ptr", "count")):
            kw["seg_ptr"] = dev(self.sp)
        q = dev(self.q) if q is None else q
        k = dev(self.k) if k is None else k
        v = dev(self.v) if v is None else v
        return ops.attention_aggregate(self.kind, q, k, dev(self.gi) if gi is None else gi, self.size, v=v,
                                       q_index=dev(self.qi), heads=self.heads, scale=self.scale,
                                       negative_slope=self.slope, **kw)


def check_forms(ops, b):
    """A: the three forms against the restatement, and each other"""
    x, alpha, out = b.want()
    got, a, lg = b.call(ops, return_attention=True, return_logits=True)
    assert same_np(lg, x), "logits"
    assert same_np(a, alpha), "alpha"
    assert same_np(got, out), "out"
    again, a2 = b.call(ops, return_attention=True)
    assert same(got, again) and same(a, a2)
    assert same(got, b.call(ops))                                      # alpha not wanted: staged
    by_keys, ak = b.call(ops, indices=dev(b.keys), return_attention=True)
    assert same(got, by_keys) and same(a, ak)
    # unsorted keys that keep the order inside a destination, and a few keys outside [0, size)
    e = b.e
    extra = 5
    slot_keys = np.concatenate([b.keys, np.array([-1, b.size, b.size + 7, -3, b.size], np.int32)])
    slot_keys = slot_keys[np.random.default_rng(e).permutation(e + extra)]
    inside = np.flatnonzero((slot_keys >= 0) & (slot_keys < b.size))
    perm = np.full(e + extra, -1, np.int64)                  # slot j holds grouped update perm[j]
    perm[inside[np.argsort(slot_keys[inside], kind="stable")]] = np.arange(e)
    gi = np.where(perm >= 0, b.gi[np.maximum(perm, 0)], 0).astype(np.int32)
    shuffled, ash = b.call(ops, gi=dev(gi), indices=dev(slot_keys), return_attention=True)
    assert same(got, shuffled)
    ash = ash.cpu().numpy()
    assert np.array_equal(ash[inside[np.argsort(slot_keys[inside], kind="stable")]].view(np.uint32),
                          alpha.view(np.uint32))
    assert not ash[perm < 0].any()                                     # no destination: alpha is 0
    return x, alpha, out


@pytest.mark.parametrize("kind", ["dot", "additive"])
@pytest.mark.parametrize("heads,d", SHAPES + LONG_ONLY)
def test_mixed_lengths_equal_the_restatement_through_every_form(EA, torch_cuda, kind, heads, d):
    b = Block(kind, heads, d, MIXED, q_index=(heads % 2 == 1))
    check_forms(EA.ops, b)


@pytest.mark.parametrize("heads,d", [(1, 128), (8, 128), (3, 15), (1, 1), (1, 512)])
def test_shared_table_equals_the_restatement_and_v_equal_k(EA, torch_cuda, heads, d):
    ops = EA.ops
    b = Block("dot", heads, d, MIXED, shared=True, q_index=True)
    check_forms(ops, b)
    # E: v=None is v=k (another tensor with the same values: the two-table path)
    one, a1 = b.call(ops, return_attention=True)
    two, a2 = b.call(ops, v=dev(b.k.copy()), return_attention=True)
    assert same(one, two) and same(a1, a2)


@pytest.mark.parametrize("count", [1, 10, 16, 17, 32, 33])
def test_uniform_count_blocks(EA, torch_cuda, count):
    ops = EA.ops
    for kind, heads, d, shared, size in (("dot", 1, 128, True, 257), ("dot", 4, 20, False, 257),
                                         ("additive", 8, 128, False, 257), ("dot", 1, 128, True, 1),
                                         ("additive", 3, 15, False, 5), ("dot", 8, 1024, True, 5)):
        b = Block(kind, heads, d, [count] * size, shared=shared)
        x, alpha, out = b.want()
        got, a = b.call(ops, count=count, return_attention=True)
        assert same_np(got, out) and same_np(a, alpha), (kind, heads, d, size)
        assert same(got, b.call(ops, count=count))
        by_ptr, ap = b.call(ops, return_attention=True)
        assert same(got, by_ptr) and same(a, ap)


def test_size_zero_and_tables_of_one_row_and_ids_past_the_table(EA, torch_cuda):
    ops = EA.ops
    b = Block("dot", 1, 4, [], shared=True)
    out, a = b.call(ops, return_attention=True)
    assert out.shape == (0, 4) and a.shape == (0, 1)
    keys = dev(np.array([3, -1, 0], np.int32))                         # size 0: every key is outside
    out, a = ops.attention_aggregate("dot", dev(b.k), dev(b.k), dev(np.zeros(3, np.int32)), 0, indices=keys,
                                     return_attention=True)
    assert out.shape == (0, 4) and not a.any()
    for kind in ("dot", "additive"):
        one = Block(kind, 4, 20, [3, 0, 40], rows=1)                   # a single row: uniform alpha
        x, alpha, out = one.want()
        got, a = one.call(ops, return_attention=True)
        assert same_np(got, out) and same_np(a, alpha)
        # int64 ids read in place; one id past the table and a negative one read the last row
        ids = Block(kind, 4, 20, [3, 0, 40, 17])
        gi64 = ids.gi.astype(np.int64)
        gi64[[1, 5]] = [ROWS, -1]
        ids.gi = gi64
        x, alpha, out = ids.want()
        got, a = ids.call(ops, return_attention=True)
        assert same_np(got, out) and same_np(a, alpha)
        clamped = ids.gi.copy()
        clamped[[1, 5]] = ROWS - 1
        assert same(got, ids.call(ops, gi=dev(clamped.astype(np.int32))))


def composition_grads(ops, b, q, k, v, alpha, G, form):
    """the gradients as the issue lists them, from the existing ops"""
    heads, size, e = b.heads, b.size, b.e
    gi, dst = dev(b.gi), dev(b.keys)
    tv = v if v is not None else k
    # da = DOT_c G[r] * v[g] in the header's order: the op's own logits with q = G, k = v, scale 1
    _, da = ops.attention_aggregate("dot", G, tv, gi, size, heads=heads, scale=1.0, return_logits=True, **form)
    # edge_softmax's backward on the saved alpha
    dl = ops._edge_softmax_raw(alpha, da.contiguous(), form.get("indices"), form.get("seg_ptr"),
                               form.get("count", 0), size, torch.float32)
    qr = dst.long() if b.qi is None else dev(b.qi)[dst.long()].long()
    if b.kind == "dot":
        ds = dl * b.scale
        gk = ops.gather_scatter("add", q, qr.int(), gi, k.shape[0], edge_weight=ds)
        dq_dst = ops.gather_segment_reduce("add", k, gi, size, edge_weight=ds,
                                           **{n: t for n, t in form.items() if n != "indices"})
    else:
        pre = k[gi.long()] if q is None else q[qr] + k[gi.long()]
        ds = torch.where(pre < 0, dl * b.slope, dl)
        gk = ops.scatter_add(ds, gi, k.shape[0])
        dq_dst = ops.scatter_add(ds, dst, size)
    gv = ops.gather_scatter("add", G, dst, gi, tv.shape[0], edge_weight=alpha)
    gq = None
    if q is not None:
        gq = dq_dst if b.qi is None else ops.scatter_add(dq_dst, dev(b.qi), q.shape[0])
    if v is None:
        return gq, gv + gk, None
    return gq, gk, gv


@pytest.mark.parametrize("kind,heads,d,shared", [("dot", 1, 128, True), ("dot", 8, 128, False), ("dot", 3, 15, True),
                                                 ("additive", 4, 20, False), ("additive", 1, 128, False),
                                                 ("dot", 1, 512, True), ("dot", 4, 4, False)])
def test_bits_against_the_existing_ops(EA, torch_cuda, kind, heads, d, shared):
    ops = EA.ops
    for lens, form_of in ((MIXED, lambda b: {"seg_ptr": dev(b.sp)}), ([10] * 40, lambda b: {"count": 10})):
        b = Block(kind, heads, d, lens, shared=shared, q_index=(d != 128))
        form = form_of(b)
        q, k, v = dev(b.q).requires_grad_(), dev(b.k).requires_grad_(), dev(b.v)
        if v is not None:
            v.requires_grad_()
        out, alpha, lg = b.call(ops, q=q, k=k, v=v, return_attention=True, return_logits=True, **form)
        assert not alpha.requires_grad and not lg.requires_grad
        assert same(alpha, ops.edge_softmax(lg, **dict(form, size=b.size)))
        tv = v if v is not None else k
        assert same(out.detach(), ops.gather_segment_reduce("add", tv.detach(), dev(b.gi), b.size, edge_weight=alpha,
                                                            **form))
        G = dev(b.grad)
        out.backward(G)
        with torch.no_grad():
            gq, gk, gv = composition_grads(ops, b, q.detach(), k.detach(), None if v is None else v.detach(),
                                           alpha, G, form)
        assert same(q.grad, gq), "grad_q"
        assert same(k.grad, gk), "grad_k"
        if v is not None:
            assert same(v.grad, gv), "grad_v"
        # and the destination side against the restatement
        ds, dq = ref.backward(b.kind, b.q, b.k, b.v, b.gi, b.sp, heads, alpha.cpu().numpy(), b.grad, q_index=b.qi,
                              scale=b.scale, slope=b.slope)
        if b.qi is None:
            assert same_np(q.grad, dq)


def shuffled_keys(b, unread_row):
    """b's updates behind unsorted scatter keys (the order inside a destination kept), plus five
    updates whose key is outside [0, size) and which gather `unread_row`; -> (keys, gi) per slot"""
    e, extra = b.e, 5
    keys = np.concatenate([b.keys, np.array([-1, b.size, b.size + 7, -3, b.size], np.int32)])
    keys = keys[np.random.default_rng(e + 1).permutation(e + extra)]
    inside = np.flatnonzero((keys >= 0) & (keys < b.size))
    perm = np.full(e + extra, -1, np.int64)                  # slot j holds grouped update perm[j]
    perm[inside[np.argsort(keys[inside], kind="stable")]] = np.arange(e)
    gi = np.where(perm >= 0, b.gi[np.maximum(perm, 0)], unread_row).astype(np.int32)
    return keys, gi


def keyed_composition_grads(ops, b, q, k, v, alpha, G, keys, gi):
    """the gradients as the issue lists them, from the existing ops, for explicit scatter keys: an
    update whose key names no destination has alpha = ds = 0; where its key is a GATHER index (rows
    of G, rows of q) the composition reads destination 0 with that weight of 0"""
    heads, size = b.heads, b.size
    tv = v if v is not None else k
    inside = (keys >= 0) & (keys < size)
    safe = torch.where(inside, keys, torch.zeros_like(keys))
    _, da = ops.attention_aggregate("dot", G, tv, gi, size, heads=heads, scale=1.0, return_logits=True, indices=keys)
    dl = ops._edge_softmax_raw(alpha, da.contiguous(), keys, None, 0, size, torch.float32)
    assert not alpha[~inside].any() and not dl[~inside].any()
    qr = safe.long() if b.qi is None else dev(b.qi)[safe.long()].long()
    if b.kind == "dot":
        ds = dl * b.scale
        gk = ops.gather_scatter("add", q, qr.int(), gi, k.shape[0], edge_weight=ds)
        dq_dst = ops.gather_scatter("add", k, gi, keys, size, edge_weight=ds)
    else:
        pre = k[gi.long()] if q is None else q[qr] + k[gi.long()]
        ds = torch.where(pre < 0, dl * b.slope, dl)
        gk = ops.scatter_add(ds, gi, k.shape[0])
        dq_dst = ops.scatter_add(ds, keys, size)
    gv = ops.gather_scatter("add", G, safe, gi, tv.shape[0], edge_weight=alpha)
    gq = dq_dst if b.qi is None else ops.scatter_add(dq_dst, dev(b.qi), q.shape[0])
    if v is None:
        return gq, gv + gk, None
    return gq, gk, gv


@pytest.mark.parametrize("kind,heads,d,shared,dv", [("dot", 1, 128, True, None), ("dot", 8, 128, False, None),
                                                    ("dot", 3, 15, True, None), ("additive", 4, 20, False, None),
                                                    ("dot", 4, 20, False, 128), ("dot", 1, 512, True, None)])
def test_gradients_through_unsorted_keys_with_keys_outside(EA, torch_cuda, kind, heads, d, shared, dv):
    """the backward with a perm: bits against the compositions, the destination side against the
    sorted form, and nothing from the updates that have no destination"""
    ops = EA.ops
    b = Block(kind, heads, d, MIXED, shared=shared, q_index=(d != 128), dv=dv)
    unread = ROWS - 1
    b.gi[b.gi == unread] = 0
    keys_np, gi_np = shuffled_keys(b, unread)
    keys, gi = dev(keys_np), dev(gi_np)
    q, k, v = dev(b.q).requires_grad_(), dev(b.k).requires_grad_(), dev(b.v)
    if v is not None:
        v.requires_grad_()
    out, alpha = b.call(ops, q=q, k=k, v=v, gi=gi, indices=keys, return_attention=True)
    G = dev(b.grad)
    out.backward(G)
    with torch.no_grad():
        gq, gk, gv = keyed_composition_grads(ops, b, q.detach(), k.detach(), None if v is None else v.detach(),
                                             alpha, G, keys, gi)
    assert same(q.grad, gq), "grad_q"
    assert same(k.grad, gk), "grad_k"
    if v is not None:
        assert same(v.grad, gv), "grad_v"
    # the updates without a destination are the only ones that gather row `unread`
    assert not k.grad[unread].any() and (v is None or not v.grad[unread].any())
    # the destination side does not see the shuffle: the bits of the seg_ptr form
    q2, k2, v2 = dev(b.q).requires_grad_(), dev(b.k).requires_grad_(), dev(b.v)
    if v2 is not None:
        v2.requires_grad_()
    out2 = b.call(ops, q=q2, k=k2, v=v2)
    out2.backward(G)
    assert same(out, out2) and same(q.grad, q2.grad)
    # sorted keys: the same call without a perm
    q3, k3, v3 = dev(b.q).requires_grad_(), dev(b.k).requires_grad_(), dev(b.v)
    if v3 is not None:
        v3.requires_grad_()
    b.call(ops, q=q3, k=k3, v=v3, indices=dev(b.keys)).backward(G)
    assert same(q2.grad, q3.grad) and same(k2.grad, k3.grad) and (v2 is None or same(v2.grad, v3.grad))


def test_two_tables_of_different_widths(EA, torch_cuda):
    """D = 20, Dv = 128, 4 heads: phases A and C have different lane layouts; forward through every
    form, gradients against the compositions"""
    ops = EA.ops
    for lens, form_of in ((MIXED, lambda b: {"seg_ptr": dev(b.sp)}), ([10] * 40, lambda b: {"count": 10})):
        b = Block("dot", 4, 20, lens, dv=128, q_index=True)
        assert b.v.shape[1] == 128 and b.k.shape[1] == 20
        check_forms(ops, b)
        form = form_of(b)
        q, k, v = dev(b.q).requires_grad_(), dev(b.k).requires_grad_(), dev(b.v).requires_grad_()
        out, alpha = b.call(ops, q=q, k=k, v=v, return_attention=True, **form)
        G = dev(b.grad)
        out.backward(G)
        with torch.no_grad():
            gq, gk, gv = composition_grads(ops, b, q.detach(), k.detach(), v.detach(), alpha, G, form)
        assert same(q.grad, gq) and same(k.grad, gk) and same(v.grad, gv)


def grads_of(b, ops, q, k, v, gi=None, **kw):
    q, k = q.detach().clone().requires_grad_(), k.detach().clone().requires_grad_()
    v = None if v is None else v.detach().clone().requires_grad_()
    b.call(ops, q=q, k=k, v=v, gi=gi, out_dtype=torch.float32, **kw).backward(dev(b.grad))
    return [t.grad for t in (q, k, v) if t is not None]


@pytest.mark.parametrize("kind,heads,d,shared", [("dot", 1, 128, True), ("dot", 4, 20, False), ("additive", 8, 128, False)])
def test_gradients_with_int64_ids_and_16_bit_tables(EA, torch_cuda, kind, heads, d, shared):
    ops = EA.ops
    b = Block(kind, heads, d, MIXED, shared=shared)
    q, k, v = dev(b.q), dev(b.k), dev(b.v)
    # int64 ids, one past the table and a negative one: the gradient flows to the last row, as
    # with the int32 rows the kernel read
    ids = b.gi.astype(np.int64)
    ids[[1, 40]] = [ROWS, -1]
    rows = ids.copy()
    rows[[1, 40]] = ROWS - 1
    for a, c in zip(grads_of(b, ops, q, k, v, gi=dev(ids)), grads_of(b, ops, q, k, v, gi=dev(rows.astype(np.int32)))):
        assert same(a, c)
    # 16-bit tables: the fp32 gradients of the widened tables, rounded once
    for dt in (torch.bfloat16, torch.float16):
        q16, k16, v16 = q.to(dt), k.to(dt), None if v is None else v.to(dt)
        wide = grads_of(b, ops, q16.float(), k16.float(), None if v16 is None else v16.float())
        for a, c in zip(grads_of(b, ops, q16, k16, v16), wide):
            assert a.dtype == dt and same(a, c.to(dt))


def test_additive_without_q_and_identity_slope(EA, torch_cuda):
    """AttentionPool: q=None, slope 1, k = the gate"""
    ops = EA.ops
    b = Block("additive", 1, 20, MIXED, with_q=False, slope=1.0)
    x, alpha, out = b.want()
    got, a = ops.attention_aggregate("additive", None, dev(b.k), dev(b.gi), b.size, v=dev(b.v), negative_slope=1.0,
                                     seg_ptr=dev(b.sp), return_attention=True)
    assert same_np(got, out) and same_np(a, alpha)
    assert same(a, ops.edge_softmax(dev(b.k)[dev(b.gi).long()], seg_ptr=dev(b.sp)))


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
def test_storage_types(EA, torch_cuda, dt):
    ops, dt = EA.ops, getattr(torch, dt)
    for kind, heads, d, shared, lens in (("dot", 1, 128, True, [10] * 33), ("dot", 4, 20, False, MIXED),
                                         ("additive", 8, 128, False, MIXED), ("dot", 3, 15, True, MIXED)):
        b = Block(kind, heads, d, lens, shared=shared)
        q, k, v = dev(b.q).to(dt), dev(b.k).to(dt), None if b.v is None else dev(b.v).to(dt)
        wide = b.call(ops, q=q.float(), k=k.float(), v=None if v is None else v.float(), return_attention=True)
        got = b.call(ops, q=q, k=k, v=v, return_attention=True, out_dtype=torch.float32)
        assert same(got[0], wide[0]) and same(got[1], wide[1])
        narrow = b.call(ops, q=q, k=k, v=v)
        assert narrow.dtype == dt and same(narrow, wide[0].to(dt))
        mixed = b.call(ops, q=q.float(), k=k, v=v, out_dtype=torch.float32)      # each table its own type
        assert same(mixed, wide[0])


@pytest.mark.parametrize("kind,heads,d", [("dot", 1, 128), ("dot", 4, 20), ("additive", 8, 128), ("dot", 1, 512)])
def test_forward_against_float64_within_the_derived_bound(EA, torch_cuda, kind, heads, d):
    b = Block(kind, heads, d, MIXED, shared=(kind == "dot" and d == 128))
    got = b.call(EA.ops).cpu().numpy().astype(np.float64)
    want, bound = ref.forward_f64(b.kind, b.q, b.k, b.v, b.gi, b.sp, heads, q_index=b.qi, scale=b.scale,
                                  slope=b.slope)
    err = np.abs(got - want)
    print("largest error / bound = %.4f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)


def test_empty_destinations_are_zero_rows_with_zero_gradients(EA, torch_cuda):
    ops = EA.ops
    for kind, shared in (("dot", True), ("additive", False)):
        b = Block(kind, 4, 20, [0, 5, 0, 0, 40, 0], shared=shared)
        q, k = dev(b.q).requires_grad_(), dev(b.k).requires_grad_()
        v = None if b.v is None else dev(b.v).requires_grad_()
        out = b.call(ops, q=q, k=k, v=v)
        empty = [0, 2, 3, 5]
        assert not out[empty].any() and bool(out[[1, 4]].any())
        out.backward(dev(b.grad))
        assert not q.grad[empty].any() and bool(q.grad[[1, 4]].any())
        unread = np.setdiff1d(np.arange(ROWS), b.gi)
        assert not k.grad[unread].any()
    none = Block("dot", 1, 4, [0, 0, 0], shared=True)                  # no update at all
    assert not none.call(ops).any()


def test_argument_errors(EA, torch_cuda):
    ops = EA.ops
    b = Block("dot", 4, 20, [3, 2])
    q, k, v, gi, sp = dev(b.q), dev(b.k), dev(b.v), dev(b.gi), dev(b.sp)
    with pytest.raises(ValueError):
        ops.attention_aggregate("dot", q, k, gi, 2, v=v, heads=4, seg_ptr=sp, count=5)         # two forms
    with pytest.raises(ValueError):
        ops.attention_aggregate("dot", q, k, gi, 2, v=v, heads=4)                              # none
    with pytest.raises(ValueError):
        ops.attention_aggregate("dot", q, k, gi, 2, v=v, heads=3, seg_ptr=sp)                  # heads, D
    with pytest.raises(ValueError):
        ops.attention_aggregate("dot", q, k, gi, 2, v=v[:, :18].contiguous(), heads=4, seg_ptr=sp)   # heads, Dv
    with pytest.raises(ValueError):
        ops.attention_aggregate("additive", q[:, :4].contiguous(), k[:, :4].contiguous(), gi, 2, heads=4, seg_ptr=sp)
    with pytest.raises(ValueError):
        ops.attention_aggregate("dot", q, k, gi, 2, v=v, heads=4, seg_ptr=sp,
                                q_index=dev(np.zeros(3, np.int32)))                            # q_index length
    with pytest.raises(ValueError):
        ops.attention_aggregate("cosine", q, k, gi, 2, v=v, heads=4, seg_ptr=sp)
    with pytest.raises(TypeError):
        ops.attention_aggregate("dot", q.double(), k.double(), gi, 2, heads=4, seg_ptr=sp)
    with pytest.raises(TypeError):
        ops.attention_aggregate("dot", q, k, gi.float(), 2, v=v, heads=4, seg_ptr=sp)
    with pytest.raises(IndexError):
        ops.attention_aggregate("dot", q, k, dev(np.full(5, ROWS, np.int32)), 2, v=v, heads=4, seg_ptr=sp,
                                validate=True)
