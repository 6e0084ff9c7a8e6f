"""Every entry that resolves its destinations through SegDest (mp_segments.h) - edge_softmax and its
gradient, segment_attention and its gradient, relation_reduce, gather_reduce_norm, and the reduces
behind scatter_ / gather_scatter / gather_segment_reduce - on the smallest blocks that sit on the
resolver's branches:
  e = 1 (no look at the keys' order), two descending keys (the sort at its smallest), two sorted keys,
  a key >= size (sorted and unsorted), a seg_ptr whose span leaves out the first and the last update,
  size = 1, count = 1, and for gather_reduce_norm a block without edges that names no form at all.
Each result has the bits of the op's numpy restatement (edge_softmax_ref, segment_attention_ref,
relation_reduce_ref, gcn_norm_ref, mp_base_ref: fp32, no tolerance - what the ops' own GPU tests
ask).  Every block is also run through each other form that can state it (the keys as they are,
seg_ptr over the grouped updates, count where the segments are equally long and span everything):
edge_softmax promises the same bits through every form, gather_scatter those of
gather_segment_reduce, and the others are held to it too."""
import numpy as np
import pytest

import edge_softmax_ref as es_ref
import gcn_norm_ref as gcn_ref
import mp_base_ref as mp_ref
import relation_reduce_ref as rel_ref
import segment_attention_ref as att_ref

pytestmark = pytest.mark.gpu

ROWS, D, HEADS, RELS = 6, 8, 2, 3
F = np.float32

# (name, form, its argument, size, e)
CASES = [
    ("one_update", "indices", [0], 1, 1),
    ("two_keys_descending", "indices", [1, 0], 2, 2),
    ("two_keys_sorted", "indices", [0, 1], 2, 2),
    ("sorted_key_past_size", "indices", [0, 0, 1, 3], 3, 4),
    ("unsorted_keys_past_size", "indices", [3, 1, 0, 0, 5], 3, 5),
    ("seg_ptr_inner_span", "seg_ptr", [1, 2, 4], 2, 5),
    ("seg_ptr_size_one", "seg_ptr", [0, 3], 1, 3),
    ("count_one", "count", 1, 3, 3),
    ("count_size_one", "count", 3, 1, 3),
]


class Block(object):
    """one case with seeded inputs: dst[p] = the destination of update p (`size`: none), and every
    form that states the same block: (kw of the op, order) - the call sees the updates in `order`"""

    def __init__(self, name, form, arg, size, e):
        self.name, self.size, self.e = name, size, e
        if form == "indices":
            self.dst = np.minimum(np.asarray(arg, np.int64), size)
            first = ({"indices": np.asarray(arg, np.int32)}, np.arange(e))
        elif form == "seg_ptr":
            sp = np.asarray(arg, np.int64)
            pos = np.arange(e)
            self.dst = np.where((pos < sp[0]) | (pos >= sp[-1]), size, np.searchsorted(sp, pos, side="right") - 1)
            first = ({"seg_ptr": sp}, pos)
        else:
            self.dst = np.repeat(np.arange(size, dtype=np.int64), arg)
            first = ({"count": int(arg)}, np.arange(e))
        # the grouped block: updates in the stable order of their destinations, those without one last
        self.order = np.argsort(self.dst, kind="stable")
        self.sp = np.searchsorted(self.dst[self.order], np.arange(size + 1), side="left").astype(np.int64)
        lens = np.diff(self.sp)
        self.forms = [first]
        if form != "indices":
            self.forms.append(({"indices": self.dst.astype(np.int32)}, np.arange(e)))
        if form != "seg_ptr":
            self.forms.append(({"seg_ptr": self.sp}, self.order))
        if form != "count" and self.sp[-1] == e and lens.min() == lens.max() and lens[0] >= 1:
            self.forms.append(({"count": int(lens[0])}, self.order))
        rng = np.random.default_rng(len(name) * 1000 + e)
        self.x = rng.uniform(-4, 4, (e, HEADS)).astype(F)               # logits
        self.g = rng.uniform(-1, 1, (e, HEADS)).astype(F)
        self.table = rng.uniform(-4, 4, (ROWS, D)).astype(F)
        self.scores = rng.uniform(-2, 2, (ROWS, HEADS)).astype(F)      # additive attention: k
        self.q = rng.uniform(-1, 1, (size, D)).astype(F)
        self.q_scores = rng.uniform(-2, 2, (size, HEADS)).astype(F)
        self.grad = rng.uniform(-1, 1, (size, D)).astype(F)
        self.gi = rng.integers(0, ROWS, e).astype(np.int32)
        self.types = rng.integers(-1, RELS + 1, e).astype(np.int32)     # -1 and RELS: no relation


BLOCKS = [Block(*c) for c in CASES]
IDS = [c[0] for c in CASES]


def test_the_cases_sit_on_the_branches():
    by = {b.name: b for b in BLOCKS}
    assert by["one_update"].e == 1 and by["one_update"].size == 1
    for name in ("two_keys_descending", "unsorted_keys_past_size"):
        k = by[name].forms[0][0]["indices"]
        assert (k[1:] < k[:-1]).any()
    for name in ("two_keys_sorted", "sorted_key_past_size"):
        k = by[name].forms[0][0]["indices"]
        assert (k[1:] >= k[:-1]).all()
    assert by["two_keys_descending"].e == 2 and by["two_keys_sorted"].e == 2
    assert (by["sorted_key_past_size"].dst == 3).sum() == 1 and (by["unsorted_keys_past_size"].dst == 3).sum() == 2
    b = by["seg_ptr_inner_span"]
    assert list(b.dst) == [2, 0, 1, 1, 2] and list(b.sp) == [0, 1, 3]
    # ... which, stated by key, is one more unsorted key array with keys >= size
    assert list(b.forms[1][0]["indices"]) == [2, 0, 1, 1, 2]
    assert [sorted(f[0])[0] for f in by["count_one"].forms] == ["count", "indices", "seg_ptr"]
    assert [sorted(f[0])[0] for f in by["one_update"].forms] == ["indices", "seg_ptr", "count"]
    assert all(len(b.forms) >= 2 for b in BLOCKS)


def dev(torch, a):
    return torch.as_tensor(a, device="cuda")


def kw_dev(torch, kw):
    return {k: (v if k == "count" else dev(torch, v)) for k, v in kw.items()}


def same_np(got, want):
    got = got.detach().cpu().numpy()
    return got.dtype == want.dtype == F and got.shape == want.shape and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


def scattered(order, grouped):
    """the rows of a grouped per-update result, back at the updates' own positions"""
    out = np.empty_like(grouped)
    out[order] = grouped
    return out


@pytest.mark.parametrize("b", BLOCKS, ids=IDS)
def test_edge_softmax_and_its_gradient(EA, torch_cuda, b):
    torch, ops = torch_cuda, EA.ops
    y = es_ref.edge_softmax_ref(b.x[b.order], b.sp)
    gx = es_ref.edge_softmax_ref(y, b.sp, b.g[b.order])
    want_y, want_gx = scattered(b.order, y), scattered(b.order, gx)
    for kw, order in b.forms:
        x = dev(torch, b.x[order]).requires_grad_()
        got = ops.edge_softmax(x, size=b.size, **kw_dev(torch, kw))
        assert same_np(got, want_y[order]), (b.name, sorted(kw))
        got.backward(dev(torch, b.g[order]))
        assert same_np(x.grad, want_gx[order]), (b.name, sorted(kw))


@pytest.mark.parametrize("kind", ["dot", "additive"])
@pytest.mark.parametrize("b", BLOCKS, ids=IDS)
def test_segment_attention_and_its_gradient(EA, torch_cuda, b, kind):
    torch, ops = torch_cuda, EA.ops
    q_np, k_np = (b.q, b.table) if kind == "dot" else (b.q_scores, b.scores)
    v_np = None if kind == "dot" else b.table           # dot: one table, read once for logit and sum
    args = dict(scale=0.37, slope=0.2)
    _, alpha, out = att_ref.forward(kind, q_np, k_np, v_np, b.gi[b.order], b.sp, HEADS, **args)
    _, dq = att_ref.backward(kind, q_np, k_np, v_np, b.gi[b.order], b.sp, HEADS, alpha, b.grad, **args)
    want_alpha = scattered(b.order, alpha)
    for kw, order in b.forms:
        q = dev(torch, q_np).requires_grad_()
        got, a = ops.attention_aggregate(kind, q, dev(torch, k_np), dev(torch, b.gi[order]), b.size,
                                         v=None if v_np is None else dev(torch, v_np), heads=HEADS, scale=0.37,
                                         negative_slope=0.2, return_attention=True, **kw_dev(torch, kw))
        assert same_np(got, out), (b.name, sorted(kw))
        assert same_np(a, want_alpha[order]), (b.name, sorted(kw))
        got.backward(dev(torch, b.grad))
        assert same_np(q.grad, dq), (b.name, sorted(kw))


@pytest.mark.parametrize("op", rel_ref.OPS)
@pytest.mark.parametrize("b", BLOCKS, ids=IDS)
def test_relation_reduce(EA, torch_cuda, b, op):
    torch, ops = torch_cuda, EA.ops
    want, want_counts = rel_ref.relation_reduce_ref(op, b.table, b.gi, b.types, RELS, b.dst, b.size)
    for kw, order in b.forms:
        got, counts = ops.relation_reduce(op, dev(torch, b.table), dev(torch, b.gi[order]), dev(torch, b.types[order]),
                                          RELS, b.size, return_counts=True, **kw_dev(torch, kw))
        assert same_np(got, want), (b.name, sorted(kw))
        assert np.array_equal(counts.cpu().numpy(), want_counts), (b.name, sorted(kw))


def gcn_edges(torch, kw, src):
    """gcn_aggregate's edge arguments of a form: (dst keys, src), or src with seg_ptr / count"""
    if "indices" in kw:
        return (dev(torch, kw["indices"]), dev(torch, src)), {}
    return dev(torch, src), kw_dev(torch, kw)


@pytest.mark.parametrize("op", ["add", "mean"])
@pytest.mark.parametrize("b", BLOCKS, ids=IDS)
def test_gather_reduce_norm(EA, torch_cuda, b, op):
    torch, ops = torch_cuda, EA.ops
    nd, ns = gcn_ref.gcn_norm(b.dst, b.gi, b.size, ROWS)
    want = gcn_ref.gcn_aggregate(op, b.table, b.dst, b.gi, b.size, nd, ns)
    assert np.abs(want).sum() > 0
    norm = (dev(torch, nd), dev(torch, ns))
    for kw, order in b.forms:
        edges, seg = gcn_edges(torch, kw, b.gi[order])
        got = ops.gcn_aggregate(dev(torch, b.table), edges, (b.size, ROWS), norm, op=op, **seg)
        assert same_np(got, want), (b.name, sorted(kw))


@pytest.mark.parametrize("op", ["add", "mean"])
def test_gather_reduce_norm_without_edges_and_without_a_form(EA, torch_cuda, op):
    """e = 0 in the key form: the keys of an empty tensor are null, so the entry sees no form at all"""
    torch, ops = torch_cuda, EA.ops
    b = BLOCKS[3]
    none = torch.zeros((2, 0), dtype=torch.int32, device="cuda")
    assert none.data_ptr() == 0
    nd, ns = np.zeros(b.size, F), np.zeros(ROWS, F)
    root = b.grad[:, :D]
    empty = np.zeros(0, np.int64)
    want = gcn_ref.gcn_aggregate(op, b.table, empty, empty, b.size, nd, ns, root=root, a=1.0, b=1.0)
    assert np.array_equal(want, root)
    got = ops.gcn_aggregate(dev(torch, b.table), none, (b.size, ROWS), (dev(torch, nd), dev(torch, ns)), op=op,
                            root=dev(torch, root))
    assert same_np(got, want)


@pytest.mark.parametrize("op", ["add", "max", "mean"])
@pytest.mark.parametrize("b", BLOCKS, ids=IDS)
def test_the_segment_reduces(EA, torch_cuda, b, op):
    """scatter_ and gather_scatter by key, gather_segment_reduce by seg_ptr or count: one answer"""
    torch, ops = torch_cuda, EA.ops
    want = mp_ref.gather_scatter_ref(op, b.table, b.gi, b.dst, b.size)
    assert same_np(torch.as_tensor(mp_ref.scatter_ref(op, b.table[b.gi], b.dst, b.size)), want)
    table = dev(torch, b.table)
    for kw, order in b.forms:
        gi = dev(torch, b.gi[order])
        if "indices" in kw:
            keys = dev(torch, kw["indices"])
            assert same_np(ops.gather_scatter(op, table, gi, keys, b.size), want), (b.name, "gather_scatter")
            assert same_np(ops.scatter_(op, table[gi.long()].contiguous(), keys, b.size), want), (b.name, "scatter")
        else:
            got = ops.gather_segment_reduce(op, table, gi, b.size, **kw_dev(torch, kw))
            assert same_np(got, want), (b.name, sorted(kw))
