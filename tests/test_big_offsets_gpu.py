"""The table and per-edge ops on buffers past 2^31 elements and 2^32 bytes: every offset the kernels
form as id * d + c, r * d + c or (t * k + j) * d, at the rows where a 32-bit product would wrap.

One flat zeroed buffer of bo.BUF elements per dtype (8.1 GiB in 16 bits, 16.3 GiB in fp32), made by
a module-scoped fixture that is parametrised over the dtype, so that one buffer is alive at a time.
A table is the view [n // d, d] of the buffer's first n = 2^32 + 2^20 elements, for d = 136, 132 and
129 (the 8-wide, 4-wide and element chunk paths).  Only the probe rows (tests/big_offsets.py: rows
0, 1, the last two, and the rows around element 2^30 / 2^31 / 2^32) hold values, all non-zero;
test_big_offsets_host.py shows that a read of such a row through a narrowed offset returns
something else.  The per-edge block is the view [2^23 + 5, 520] of the whole buffer (that block is
what bo.BUF is sized for: it is 1.6 % more than 2^32 + 2^20 elements).

Expected values never come from the op under test nor from a host copy of the big table: they are
the op's existing independent reference on the small table of the probe rows with the ids
renumbered (big_offsets.compact), compared as the op's own GPU test compares - bits wherever the
contract says bits, the bound of test_weighted_mp_gpu.py for edge_dot.  After every case the
non-zero elements of the whole buffer are counted in chunks of 2^30: a read-only op leaves exactly
what was written, a writer exactly the non-zero elements of the expected table, so a store through
a narrowed offset is seen wherever it lands; big outputs and state tensors are counted likewise.

Covered, each over bf16 / fp16 / fp32 and the three d:
  read by row    gather; gather_scatter and gather_segment_reduce (add, max, mean; count, seg_ptr,
                 int64 ids; edge weights); gather_segment_topk with indices; edge_dot; gcn_aggregate;
                 attention_aggregate; relation_reduce; embedding_take; sparse_feature_embedding
  scanned whole  table_topk (k = 64; the four metrics at d = 136, ip and l2 at 132 and 129; with and
                 without exclude, once with ids=) and table_rank over all 31.6 M rows (the three
                 dtypes, the three d): 33 queries in a second dtype - two query tiles, the
                 cap of 512 slabs and the merge over 512 * 64 entries a query; expected values from
                 table_search_ref.sparse_topk / sparse_rank on the probe rows
  sparse grads  triple_score, triple_score_proj (TransD with a second big table), triple_score_matrix,
                 skipgram_loss (the big table as target, then as context)
  written        embedding_update / _add / _take(clear) in the plain, row_index and count forms, once
                 on a side stream; sparse_row_step sgd / momentum / adagrad with a 16 GiB state tensor
                 and adam with two 8 GiB ones over a table of 2^31 + 2^20 elements
  per-edge block scatter_add / _max / _mean of big updates; gather and embedding_take into a big
                 output; the top-k gradient entry with size * k * d >= 2^32; the dense gradient of
                 gather, a scatter_add into [rows, d] past 2^32 elements
Not covered: scatter_softmax of a big block - its fp32 composition holds four [e, 520] fp32
temporaries (65 GiB) at once - and the top-k gradient through autograd, whose forward would add an
[e, 520] fp32 per-edge block to out, sel and grad; its entry is called directly instead."""
import contextlib

import numpy as np
import pytest

import big_offsets as bo
import embed_store_ref as store_ref
import gcn_norm_ref as G
import mp_base_ref as R
import relation_reduce_ref as RR
import segment_attention_ref as A
import segment_topk_ref as TK
import skipgram_ref as SG
import sparse_embed_ref as SE
import sparse_optim_ref as SO
import table_search_ref as SR
import triple_score_matrix_ref as TM
import triple_score_proj_ref as TP
import triple_score_ref as TS
import weighted_mp_ref as W

pytestmark = pytest.mark.gpu

DTYPES = store_ref.DTYPES
GIB = 1 << 30
# the most a test holds at once (41.6 GiB measured), with a margin: the fp32 buffer (16.3 GiB), beside it
# the fp32 [2^23 + 5, 520] block a gather writes (16.3 GiB) - or the int32 sel of the top-k gradient, or
# a state tensor of the table's shape - and the 9 GiB torch.count_nonzero takes for a chunk of 2^30
# elements; in 16 bits the buffer (8.1), the dense fp32 gradient of a table (16) and its rounded copy (8)
NEED = 44 * GIB
MODES = ["add", "max", "mean"]
HEADS = {136: 4, 132: 3, 129: 3}


def tdt(torch, dt):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dt]


def dt_of(torch, t):
    return {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}[t.dtype]


def int_view(torch, t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def host(torch, t):
    """a cuda tensor -> its numpy storage (float32, or uint16 bits)"""
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def dev(torch, a, dt="f32"):
    """numpy storage (float32 / uint16 bits / integers) -> a cuda tensor"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(tdt(torch, dt))
    return torch.from_numpy(a).cuda()


def nonzero_bits(a):
    a = np.ascontiguousarray(a)
    return int(np.count_nonzero(a.view(np.uint32 if a.dtype == np.float32 else np.uint16)))


def stored_as(want32, torch, out):
    """a float32 expected array in the storage of the tensor `out`: one rounding to nearest even"""
    return store_ref.narrow(np.asarray(want32, np.float32), dt_of(torch, out))


def same(torch, got, want32):
    """got (a cuda tensor) has the shape of want32 and the bits of want32 rounded once to its dtype"""
    want = stored_as(want32, torch, got)
    return tuple(got.shape) == want.shape and store_ref.same(host(torch, got), want)


class Table:
    """the view [n // d, d] of a buffer's first n elements, and what its probe rows hold"""

    def __init__(self, torch, buf, dt, d, n_elems, seed):
        self.torch, self.dt, self.d = torch, dt, d
        self.rows = n_elems // d
        self.t = buf[:self.rows * d].view(self.rows, d)
        assert self.t.is_contiguous() and self.t.data_ptr() == buf.data_ptr()
        self.probe = bo.probe_rows(n_elems, d, bo.ELEM_BYTES[dt])
        self.probe_t = torch.from_numpy(self.probe).cuda()
        self.values = bo.probe_values(np.random.default_rng(seed), len(self.probe), d)     # float32, exact in dt
        self.small = store_ref.narrow(self.values, dt)                                    # the storage of dt
        self.nnz = self.values.size

    def write(self):
        self.t[self.probe_t] = dev(self.torch, self.small, self.dt)

    def read(self):
        """the probe rows as they are on the device -> numpy storage"""
        return host(self.torch, self.t[self.probe_t])

    def zero(self):
        self.t[self.probe_t] = 0

    def compact(self, ids):
        return bo.compact(ids, self.probe, self.rows)

    def ids(self, rng, extra=(), total=64, repeat=2):
        return bo.named_twice(rng, self.probe, extra, repeat, total)


class Big:
    def __init__(self, torch, dt):
        self.torch, self.dt = torch, dt
        self.buf = torch.zeros(bo.BUF, dtype=tdt(torch, dt), device="cuda")
        assert self.buf.data_ptr() % 16 == 0

    def count(self):
        """the elements of the whole buffer whose bits are not zero, in chunks of 2^30"""
        v = int_view(self.torch, self.buf)
        total = self.torch.zeros((), dtype=self.torch.int64, device="cuda")
        for lo in range(0, v.numel(), 1 << 30):
            total += self.torch.count_nonzero(v[lo:lo + (1 << 30)])
        return int(total)

    @contextlib.contextmanager
    def table(self, d, n_elems=bo.BIG, seed=None):
        """a table with its probe rows written; zeroed again on the way out, whatever happened"""
        t = Table(self.torch, self.buf, self.dt, d, n_elems, d if seed is None else seed)
        t.write()
        try:
            yield t
        finally:
            t.zero()
        assert self.count() == 0


@pytest.fixture(scope="module", params=DTYPES)
def big(request, torch_cuda):
    """one flat zeroed buffer of the parameter's dtype; freed before the next dtype's is made"""
    torch = torch_cuda
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < NEED:
        pytest.skip("tables past 2^32 elements need %d GiB of free GPU memory, %.1f GiB are free"
                    % (NEED // GIB, free / GIB))
    torch.cuda.reset_peak_memory_stats()
    b = Big(torch, request.param)
    yield b
    print("\n[big offsets %s] peak memory allocated %.1f GiB" % (request.param, torch.cuda.max_memory_allocated() / GIB))
    b.buf = None
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def ops(EA):
    return EA.ops


def out_dtypes(torch, dt):
    return (None,) if dt == "f32" else (None, torch.float32)


# ---- the table read by row index --------------------------------------------------------------
@pytest.mark.parametrize("d", bo.DIMS)
def test_gather(big, ops, d):
    torch = big.torch
    rng = np.random.default_rng(1000 + d)
    with big.table(d) as t:
        ids = t.ids(rng)
        want = R.gather_ref(t.values, t.compact(ids))
        for od in out_dtypes(torch, big.dt):
            for idx in (dev(torch, ids), dev(torch, ids.astype(np.int32))):
                assert same(torch, ops.gather(t.t, idx, out_dtype=od), want), (d, od)
        assert big.count() == t.nnz


def edge_case(t, rng, size=37, count=3):
    """ids [size * count] that name every probe row twice, keys with empty destinations and keys that
    name none, a seg_ptr with empty segments, exact weights"""
    e = size * count
    ids = t.ids(rng, total=e)
    keys = rng.integers(0, size, e).astype(np.int32)
    keys[keys == 5] = 6                                               # destination 5 stays empty
    keys[::11] = -1
    keys[3::17] = size
    keys[4::19] = size + 5
    lens = rng.multinomial(e, np.ones(size) / size)
    lens[[0, 9]] = 0
    lens[-1] += e - lens.sum()
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert ptr[-1] == e
    w = (rng.integers(-8, 9, (e, HEADS[t.d])) / 4).astype(np.float32)
    return e, ids, keys, ptr, w


@pytest.mark.parametrize("d", bo.DIMS)
@pytest.mark.parametrize("op", MODES)
def test_gather_scatter_and_segment_reduce(big, ops, op, d):
    """gather_scatter and gather_segment_reduce (count, seg_ptr; int32 rows and int64 ids read in
    place), with and without edge weights: the bits of the sequential fp32 loop"""
    torch = big.torch
    rng = np.random.default_rng(2000 + d)
    size, count = 37, 3
    with big.table(d) as t:
        e, ids, keys, ptr, w = edge_case(t, rng, size, count)
        # the int64 form reads the low word, capped at the last row: -1, rows + 5 and 2^33 + row
        wide = ids.copy()
        wide[1::7] += 1 << 33
        wide[2::13] = -1
        wide[9::13] = t.rows + 5
        small = t.compact(ids)
        small_wide = t.compact(R.id_rows(wide, t.rows))
        assert (small_wide != small).any()
        by_count, by_ptr = R.segment_keys(size, count=count), R.segment_keys(size, seg_ptr=ptr)
        gi, gw = dev(torch, ids.astype(np.int32)), dev(torch, wide)
        kt, pt, wt = dev(torch, keys), dev(torch, ptr), dev(torch, w)
        x = t.values
        for od in out_dtypes(torch, big.dt):
            why = (op, d, od)
            assert same(torch, ops.gather_scatter(op, t.t, gi, kt, size, out_dtype=od),
                        R.gather_scatter_ref(op, x, small, keys, size)), why
            assert same(torch, ops.gather_segment_reduce(op, t.t, gi, size, count=count, out_dtype=od),
                        R.gather_scatter_ref(op, x, small, by_count, size)), why
            assert same(torch, ops.gather_segment_reduce(op, t.t, gi, size, seg_ptr=pt, out_dtype=od),
                        R.gather_scatter_ref(op, x, small, by_ptr, size)), why
            assert same(torch, ops.gather_segment_reduce(op, t.t, gw, size, count=count, out_dtype=od),
                        R.gather_scatter_ref(op, x, small_wide, by_count, size)), why
            assert same(torch, ops.gather_segment_reduce(op, t.t, gw, size, seg_ptr=pt, out_dtype=od),
                        R.gather_scatter_ref(op, x, small_wide, by_ptr, size)), why
            # weighted
            assert same(torch, ops.gather_scatter(op, t.t, gi, kt, size, out_dtype=od, edge_weight=wt),
                        W.gather_scatter_ref(op, x, small, np.where(R.valid_keys(keys, size), keys, size), size, w)), why
            assert same(torch, ops.gather_segment_reduce(op, t.t, gi, size, count=count, out_dtype=od, edge_weight=wt),
                        W.gather_scatter_ref(op, x, small, by_count, size, w)), why
            assert same(torch, ops.gather_segment_reduce(op, t.t, gw, size, seg_ptr=pt, out_dtype=od, edge_weight=wt),
                        W.gather_scatter_ref(op, x, small_wide, by_ptr, size, w)), why
        assert big.count() == t.nnz


# ---- the table written in place ---------------------------------------------------------------
def store_case(t, rng, form):
    """(ids, values float32, row_index, count): every probe row named at least twice, ids that name no
    row among them"""
    count = 4 if form == "count" else None
    ids = t.ids(rng, extra=bo.no_row_ids(t.rows) * 2, total=96)
    m = {"plain": len(ids), "row_index": 9, "count": len(ids) // 4}[form]
    values = bo.probe_values(rng, m, t.d)
    ri = None
    if form == "row_index":
        ri = rng.integers(0, m, len(ids)).astype(np.int32)
        ri[[3, 40, 41]] = [-1, m, 2 ** 31 - 1]
    return ids, values, ri, count


def run_store_ops(big, ops, t, rng, form, vdt):
    """update, add, take and take + clear one after the other on the same table: after each the probe
    rows have the bits of the restatement and the buffer holds nothing else"""
    torch, dt, ref = big.torch, big.dt, store_ref
    ids, values, ri, count = store_case(t, rng, form)
    small_ids = t.compact(ids)
    v = ref.narrow(values, vdt)
    t_ids, t_v = dev(torch, ids), dev(torch, v, vdt)
    t_ri = None if ri is None else dev(torch, ri)
    now = t.small
    for name, fn, want in (("update", ops.embedding_update, ref.update), ("add", ops.embedding_add, ref.add)):
        assert fn(t.t, t_ids, t_v, row_index=t_ri, count=count) is t.t
        now = want(now, dt, small_ids, v, vdt, ri, count)
        assert ref.same(t.read(), now), (name, form, t.d, vdt)
        assert big.count() == nonzero_bits(now), (name, form, t.d, vdt)
    for clear in (False, True):
        for odt in ("f32", dt):
            if clear and odt != dt:
                continue
            out = ops.embedding_take(t.t, t_ids, clear=clear, out_dtype=tdt(torch, odt))
            want_out, after = ref.take(now, dt, small_ids, clear, odt)
            assert out.shape == (len(ids), t.d) and ref.same(host(torch, out), want_out), ("take", clear, form, t.d)
            assert ref.same(t.read(), after) and big.count() == nonzero_bits(after), ("take", clear, form, t.d)
            now = after
    assert nonzero_bits(now) < t.nnz


@pytest.mark.parametrize("d", bo.DIMS)
@pytest.mark.parametrize("form", ["plain", "row_index", "count"])
def test_embedding_stores(big, ops, form, d):
    rng = np.random.default_rng(3000 + d)
    with big.table(d) as t:
        run_store_ops(big, ops, t, rng, form, "f32" if form != "row_index" else big.dt)


def test_embedding_stores_on_a_side_stream(big, ops):
    torch = big.torch
    rng = np.random.default_rng(3500)
    side = torch.cuda.Stream()
    with big.table(136) as t:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run_store_ops(big, ops, t, rng, "count", "f32")
        side.synchronize()
        torch.cuda.current_stream().wait_stream(side)


# ---- the sparse-row optimiser steps ------------------------------------------------------------
HYPER = dict(lr=0.05, momentum=0.9, betas=(0.9, 0.999))                 # those of test_sparse_optim_gpu.py
STEP_FORM = {"sgd": "plain", "momentum": "count", "adagrad": "row_index", "adam": "plain"}


def count_all(torch, t):
    v = int_view(torch, t.reshape(-1))
    return sum(int(torch.count_nonzero(v[lo:lo + (1 << 30)])) for lo in range(0, v.numel(), 1 << 30))


@pytest.mark.parametrize("d", bo.DIMS)
@pytest.mark.parametrize("kind", SO.KINDS)
def test_sparse_row_step(big, ops, kind, d):
    """two steps, so that the second reads the state the first wrote: the table and the fp32 state
    tensors (of the table's shape: 16 GiB each; Adam's two over a table of 2^31 + 2^20 elements) have
    the bits of the restatement in the probe rows and nothing anywhere else"""
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(4000 + d)
    with big.table(d, bo.HALF if kind == "adam" else bo.BIG) as t:
        ids, grad, ri, count = store_case(t, rng, STEP_FORM[kind])
        gdt = dt if kind in ("sgd", "adam") else "f32"
        g = store_ref.narrow(grad, gdt)
        small_ids = t.compact(ids)
        state = [torch.zeros(t.t.shape, dtype=torch.float32, device="cuda") for _ in range(SO.N_STATE[kind])]
        t_ids, t_g, t_ri = dev(torch, ids), dev(torch, g, gdt), None if ri is None else dev(torch, ri)
        now, st = t.small, [np.zeros(t.values.shape, np.float32) for _ in state]
        for step in (1, 2):
            assert ops.sparse_row_step(kind, t.t, t_ids, t_g, state, step=step, row_index=t_ri, count=count,
                                       **HYPER) is t.t
            now, st = SO.step(kind, now, dt, st, small_ids, g, gdt, SO.scalars(kind, step=step, **HYPER), ri, count)
            why = (kind, d, step)
            assert store_ref.same(t.read(), now) and big.count() == nonzero_bits(now), why
            for got, want in zip(state, st):
                assert store_ref.same(host(torch, got[t.probe_t]), want) and count_all(torch, got) == nonzero_bits(want), why
        del state


# ---- the table read with sparse gradients -----------------------------------------------------
KG_KINDS, CORRUPTS = ("trans_l1", "trans_l2", "distmult"), ("front", "tail", "both")


def np_same(got, want):
    """a cuda tensor has the dtype, shape and bits of a float32 / int32 numpy array"""
    got = got.detach().cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


def check_sparse_grad(torch, g, t, ids, rows):
    """g, the gradient of the big table t: a sparse_coo_tensor whose indices are the original row
    numbers of the live ids and whose values are the occurrences' fp32 rows added in occurrence
    order and rounded once"""
    ids = np.asarray(ids, np.int64).reshape(-1)
    assert g.is_sparse and tuple(g.shape) == (t.rows, t.d) and g.dtype == tdt(torch, t.dt)
    g = g.coalesce()
    idx = g.indices()[0].cpu().numpy()
    live = (ids >= 0) & (ids < t.rows)
    assert np.array_equal(idx, np.unique(ids[live])) and np.array_equal(idx, t.probe)
    want = TS.scatter_rows(np.ascontiguousarray(rows, np.float32).reshape(len(ids), t.d), t.compact(ids), len(t.probe))
    assert store_ref.same(host(torch, g.values()), store_ref.narrow(want[t.compact(idx)], t.dt))


@pytest.mark.parametrize("d", bo.DIMS)
@pytest.mark.parametrize("kind", KG_KINDS)
def test_triple_score_sparse_grad(big, ops, kind, d):
    """forward and per-occurrence gradient bits of the restatement; ent.grad sparse over the probe rows"""
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(5000 + d)
    b, k, n_rel = 32, 3, 7
    n = bo.DIMS.index(d) + KG_KINDS.index(kind)
    corrupt, normalize = CORRUPTS[n % 3], n % 2 == 0
    with big.table(d) as t:
        ids = t.ids(rng, extra=bo.no_row_ids(t.rows), total=b * (2 + k))
        src, dst, neg = ids[:b], ids[b:2 * b], ids[2 * b:].reshape(b, k)
        rel_id = rng.integers(0, n_rel, b)
        rel_id[[3, 9]] = [-1, n_rel + 2]
        rel32 = bo.probe_values(rng, n_rel, d)
        rel = dev(torch, store_ref.narrow(rel32, dt), dt)
        ent = t.t.detach().requires_grad_()
        v = TS.chunk_width(d, ent.data_ptr(), ent.element_size(), rel.data_ptr(), rel.element_size())
        assert v == (8 if d % 8 == 0 else 4 if d % 4 == 0 else 1)
        pos, out = ops.triple_score(ent, rel, dev(torch, src), dev(torch, rel_id), dev(torch, dst), dev(torch, neg),
                                    kind=kind, corrupt=corrupt, normalize=normalize, sparse_grad=True)
        small = (t.compact(src), rel_id, t.compact(dst), t.compact(neg))
        want = TS.forward(t.values, rel32, *small, kind, corrupt, normalize, v)
        assert np_same(pos, want[0]) and np_same(out, want[1]), (kind, corrupt, normalize, d)
        g_pos = (rng.random(b) * 8 - 4).astype(np.float32)
        g_neg = (rng.random(want[1].shape) * 8 - 4).astype(np.float32)
        ((pos * dev(torch, g_pos)).sum() + (out * dev(torch, g_neg)).sum()).backward()
        gs, _, gd, gn = TS.grad(t.values, rel32, *small, kind, corrupt, normalize, v, g_pos, g_neg)
        check_sparse_grad(torch, ent.grad, t, np.concatenate([src, dst, neg.reshape(-1)]),
                          np.concatenate([gs, gd, gn.reshape(-1, d)]))
        assert big.count() == t.nnz


@pytest.mark.parametrize("d", bo.DIMS)
@pytest.mark.parametrize("which", ["target", "context"])
def test_skipgram_loss_sparse_grad(big, ops, which, d):
    """the big table as the target table, then as the context table; the other one has 50 rows"""
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(6000 + d)
    b, p, k, n_small = 40, 2, 3, 50
    with big.table(d) as t:
        other32 = bo.probe_values(rng, n_small, d) / 64
        other = dev(torch, store_ref.narrow(other32, dt), dt)
        assert np.array_equal(store_ref.widen(store_ref.narrow(other32, dt), dt), other32)
        few = rng.integers(-1, n_small + 1, b * (p + k) if which == "target" else b)
        many = t.ids(rng, extra=bo.no_row_ids(t.rows), total=b if which == "target" else b * (p + k))
        big_leaf = t.t.detach().requires_grad_()
        if which == "target":
            src, ctx, tables, tables32 = many, few.reshape(b, p + k), (big_leaf, other), (t.values, other32)
            small_ids = (t.compact(src), ctx[:, :p], ctx[:, p:])
        else:
            src, ctx, tables, tables32 = few, many.reshape(b, p + k), (other, big_leaf), (other32, t.values)
            small_ids = (src, t.compact(ctx[:, :p]), t.compact(ctx[:, p:]))
        v = SG.chunk_width(d, tables[0].data_ptr(), tables[0].element_size(), tables[1].data_ptr(),
                           tables[1].element_size())
        loss, rank, logits = ops.skipgram_loss(*tables, dev(torch, src), dev(torch, np.ascontiguousarray(ctx[:, :p])),
                                               dev(torch, np.ascontiguousarray(ctx[:, p:])), sparse_grad=True,
                                               return_logits=True)
        want = SG.forward(*tables32, *small_ids, v)
        assert np_same(logits, want[0]) and np_same(rank, want[1]), (which, d)
        assert np_same(loss.reshape(1), np.array([want[3]], np.float32)), (which, d)
        (loss * 0.75).backward()
        gs, gp, gn = SG.grad(*tables32, *small_ids, want[0], 0.75)
        if which == "target":
            check_sparse_grad(torch, big_leaf.grad, t, src, gs)
        else:
            check_sparse_grad(torch, big_leaf.grad, t, np.concatenate([ctx[:, :p].reshape(-1), ctx[:, p:].reshape(-1)]),
                              np.concatenate([gp.reshape(-1, d), gn.reshape(-1, d)]))
        assert big.count() == t.nnz


# ---- per-column top-k -------------------------------------------------------------------------
@pytest.mark.parametrize("d", bo.DIMS)
def test_gather_segment_topk(big, ops, d):
    """count and seg_ptr forms over int64 ids (some name no row: a candidate row of +0), out and sel"""
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(7000 + d)
    size, count, k = 16, 6, 4
    with big.table(d) as t:
        ids = t.ids(rng, extra=bo.no_row_ids(t.rows), total=size * count)
        small = t.compact(ids)
        ptr = np.concatenate([[0], np.sort(rng.integers(0, len(ids) + 1, size - 1)), [len(ids)]]).astype(np.int64)
        ptr[3] = ptr[2]
        ptr[1:] = np.maximum.accumulate(ptr[1:])
        for od in ("f32", dt):
            for kw, small_kw in ((dict(count=count), dict(count=count)), (dict(seg_ptr=dev(torch, ptr)), dict(seg_ptr=ptr))):
                out, sel = ops.gather_segment_topk(t.t, dev(torch, ids), size, k, fill=-7.0, out_dtype=tdt(torch, od),
                                                   return_indices=True, **kw)
                want_out, want_sel = TK.topk(t.small, dt, small, size, k, fill=-7.0, out_dt=od, **small_kw)
                assert TK.same(host(torch, out), want_out, od), (d, od, sorted(kw))
                assert np.array_equal(sel.cpu().numpy(), want_sel), (d, od, sorted(kw))
        assert big.count() == t.nnz


# ---- a per-edge block past 2^32 elements: e = 2^23 + 5 rows of 520 -----------------------------
def edge_probe(dts):
    """the probe rows of a [EDGE_ROWS, 520] block for every element size among dts"""
    rows = set()
    for dt in dts:
        rows |= set(bo.probe_rows(bo.EDGE_ROWS * bo.EDGE_DIM, bo.EDGE_DIM, bo.ELEM_BYTES[dt]).tolist())
    return np.array(sorted(rows), np.int64)


@pytest.mark.parametrize("op", MODES)
def test_scatter_of_a_big_edge_block(big, ops, op):
    """updates [2^23 + 5, 520] in the buffer: the probe rows and a handful of zero rows have a
    destination, every other key names none"""
    torch = big.torch
    rng = np.random.default_rng(8000)
    size = 11
    with big.table(bo.EDGE_DIM, bo.EDGE_ROWS * bo.EDGE_DIM) as t:
        e = t.rows
        assert e == bo.EDGE_ROWS and e * t.d >= 1 << 32
        zero_rows = np.array([7, e // 2 + 3, e - 9])
        assert not np.isin(zero_rows, t.probe).any()
        live = np.sort(np.concatenate([t.probe, zero_rows]))
        keys_small = rng.integers(0, size - 1, len(live)).astype(np.int32)      # the last destination stays empty
        x_small = np.zeros((len(live), t.d), np.float32)
        x_small[np.isin(live, t.probe)] = t.values
        keys = torch.full((e,), -1, dtype=torch.int32, device="cuda")
        keys[1::3] = size
        keys[2::3] = size + 5
        keys[dev(torch, live)] = dev(torch, keys_small)
        want = R.scatter_ref(op, x_small, keys_small, size)
        for od in out_dtypes(torch, big.dt):
            assert same(torch, ops.scatter_(op, t.t, keys, size, out_dtype=od), want), (op, od)
        assert big.count() == t.nnz


def small_table(torch, rng, dt, rows=40, d=bo.EDGE_DIM):
    """an ordinary table whose row 0 is zero -> (float32 values, the cuda tensor)"""
    v = bo.probe_values(rng, rows, d)
    v[0] = 0
    return v, dev(torch, store_ref.narrow(v, dt), dt)


@pytest.mark.parametrize("op", ["gather", "embedding_take"])
def test_a_big_block_written_from_a_small_table(big, ops, op):
    """out [2^23 + 5, 520]: every index reads the zero row (gather) or names no row
    (embedding_take) except at the probe positions of the output"""
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(8100)
    e, d = bo.EDGE_ROWS, bo.EDGE_DIM
    values, table = small_table(torch, rng, dt)
    for od in out_dtypes(torch, dt):
        probe = edge_probe([dt if od is None else "f32"])
        at = dev(torch, probe)
        pick = rng.integers(1, len(values), len(probe))
        if op == "gather":
            idx = torch.zeros(e, dtype=torch.int32, device="cuda")
            idx[at] = dev(torch, pick.astype(np.int32))
            out = ops.gather(table, idx, out_dtype=od)
        else:
            idx = torch.full((e,), -1, dtype=torch.int64, device="cuda")
            idx[1::3] = len(values)
            idx[2::3] = (1 << 33) + 5
            idx[at] = dev(torch, pick)
            out = ops.embedding_take(table, idx, out_dtype=od)
        assert tuple(out.shape) == (e, d) and out.numel() >= 1 << 32
        assert same(torch, out[at], values[pick]), (op, od)
        assert count_all(torch, out) == len(probe) * d, (op, od)
        del out
    assert big.count() == 0


def test_topk_gradient_past_2_32_selected_elements(big, ops):
    """euler_gpu_segment_topk_grad with size * k * d >= 2^32 (the 64-bit column arithmetic of
    TkGradKernel): grad [2^19, 16, 520] is a view of the buffer with values in its probe rows, sel is
    -1 everywhere else; every selected element lands once in the per-edge block [e, 520]"""
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(8200)
    k, d = 16, bo.EDGE_DIM
    size = bo.EDGE_ROWS // k
    assert size * k * d >= 1 << 32
    with big.table(d, size * k * d) as t:
        n = len(t.probe)
        e = 3 * n
        # element (row R, column c) goes to position first[R] + (c % 3) * n: one writer per (position, column)
        first = rng.permutation(n)
        sel_small = (first[:, None] + (np.arange(d)[None, :] % 3) * n).astype(np.int32)
        sel = torch.full((size * k, d), -1, dtype=torch.int32, device="cuda")
        sel[t.probe_t] = dev(torch, sel_small)
        got = ops._segment_topk_grad_raw(t.t.view(size, k, d), sel.view(size, k, d), e)
        want = TK.per_edge(t.values.reshape(n, 1, d), sel_small.reshape(n, 1, d), e)
        assert np_same(got, want) and np.count_nonzero(want) == t.nnz
        del sel
        assert big.count() == t.nnz


@pytest.mark.parametrize("d", bo.DIMS)
def test_gather_backward_into_a_dense_table_gradient(big, ops, d):
    """the one dense table gradient: the backward of gather is a scatter_add into [rows, d] past 2^32
    elements (fp32, then rounded once to the table's dtype)"""
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(8300 + d)
    with big.table(d) as t:
        leaf = t.t.detach().requires_grad_()
        ids = t.ids(rng)
        g32 = bo.probe_values(rng, len(ids), d)
        ops.gather(leaf, dev(torch, ids.astype(np.int32))).backward(dev(torch, store_ref.narrow(g32, dt), dt))
        grad = leaf.grad
        assert tuple(grad.shape) == (t.rows, d) and grad.dtype == tdt(torch, dt) and grad.numel() >= 1 << 32
        want = R.gather_grad(g32, t.compact(ids), len(t.probe))
        assert same(torch, grad[t.probe_t], want)
        assert count_all(torch, grad) == nonzero_bits(store_ref.narrow(want, dt))
        leaf.grad = None
        del grad, leaf
        assert big.count() == t.nnz


# ---- the other ops that read a table by row ----------------------------------------------------
@pytest.mark.parametrize("d", bo.DIMS)
def test_edge_dot(big, ops, d):
    """a and b both the big table, read at different rows: within the bound of
    test_weighted_mp_gpu.py (the values are multiples of 2^-5, so every fp32 sum here is exact)"""
    from test_weighted_mp_gpu import dot_bound, within
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(9000 + d)
    with big.table(d) as t:
        ai, bi = t.ids(rng), t.ids(rng)
        a_rows, b_rows = dev(torch, t.values[t.compact(ai)]), dev(torch, t.values[t.compact(bi)])
        for heads in (1, HEADS[d]):
            for od in (torch.float32, tdt(torch, dt)):
                got = ops.edge_dot(t.t, dev(torch, ai.astype(np.int32)), t.t, dev(torch, bi.astype(np.int32)),
                                   heads=heads, out_dtype=od)
                assert got.shape == (len(ai), heads) and got.dtype == od
                want, bound = dot_bound(torch, a_rows, b_rows, heads, od)
                assert within(torch, got, want, bound), (d, heads, od)
        assert big.count() == t.nnz


@pytest.mark.parametrize("d", bo.DIMS)
@pytest.mark.parametrize("op", ["add", "mean"])
def test_gcn_aggregate(big, ops, op, d):
    """x is the big table: keyed and count forms, with a root term; the norm tables are computed by
    the call over all the table's rows"""
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(9100 + d)
    size, count = 37, 3
    with big.table(d) as t:
        e, ids, keys, ptr, _ = edge_case(t, rng, size, count)
        small = t.compact(ids)
        src = dev(torch, ids.astype(np.int32))
        root32 = bo.probe_values(rng, size, d)
        root = dev(torch, root32)
        by_count = G.segment_dst(size, count=count)
        for od in out_dtypes(torch, dt):
            for dst_np, kw, edges in ((keys, {}, (dev(torch, keys), src)), (by_count, dict(count=count), src)):
                nd, ns = G.gcn_norm(dst_np, small, size, len(t.probe))
                got = ops.gcn_aggregate(t.t, edges, (size, t.rows), op=op, out_dtype=od, **kw)
                assert same(torch, got, G.gcn_aggregate(op, t.values, dst_np, small, size, nd, ns)), (op, d, od, sorted(kw))
                got = ops.gcn_aggregate(t.t, edges, (size, t.rows), op=op, root=root, alpha=0.25, out_dtype=od, **kw)
                want = G.gcn_aggregate(op, t.values, dst_np, small, size, nd, ns, root32, np.float32(0.75), np.float32(0.25))
                assert same(torch, got, want), (op, d, od, sorted(kw), "root")
        assert big.count() == t.nnz


@pytest.mark.parametrize("d", bo.DIMS)
@pytest.mark.parametrize("shared", [True, False])
def test_attention_aggregate(big, ops, shared, d):
    """dot attention with k (and v: the same view passed again, or v=None) the big table: logits,
    alpha and out have the bits of the restatement"""
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(9200 + d)
    size, count, heads = 37, 3, HEADS[d]
    with big.table(d) as t:
        e, ids, _, ptr, _ = edge_case(t, rng, size, count)
        small = t.compact(ids)
        q32 = bo.probe_values(rng, size, d) / 64
        q = dev(torch, q32)
        v = None if shared else t.t
        for gi in (dev(torch, ids), dev(torch, ids.astype(np.int32))):
            for od in (torch.float32, tdt(torch, dt)):
                got, alpha, lg = ops.attention_aggregate("dot", q, t.t, gi, size, v=v, heads=heads, scale=0.37,
                                                         seg_ptr=dev(torch, ptr), out_dtype=od, return_attention=True,
                                                         return_logits=True)
                x, a, out = A.forward("dot", q32, t.values, None if shared else t.values, small, ptr, heads, scale=0.37)
                assert np_same(lg, x) and np_same(alpha, a) and same(torch, got, out), (d, shared, od)
        assert big.count() == t.nnz


@pytest.mark.parametrize("d", bo.DIMS)
@pytest.mark.parametrize("op", RR.OPS)
def test_relation_reduce(big, ops, op, d):
    """keyed and count forms, int32 rows and int64 ids read in place, types that name no relation"""
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(9300 + d)
    size, count, n_rel = 37, 3, 4
    with big.table(d) as t:
        e, ids, keys, _, _ = edge_case(t, rng, size, count)
        wide = ids.copy()
        wide[1::7] += 1 << 33
        wide[2::13] = -1
        small, small_wide = t.compact(ids), t.compact(R.id_rows(wide, t.rows))
        types = rng.integers(0, n_rel, e).astype(np.int32)
        types[::9] = -1
        types[4::23] = n_rel
        by_count = RR.segment_dst(size, count=count)
        tt = dev(torch, types)
        for od in out_dtypes(torch, dt):
            for gi, sm in ((dev(torch, ids.astype(np.int32)), small), (dev(torch, wide), small_wide)):
                for dst_np, kw in ((keys, dict(indices=dev(torch, keys))), (by_count, dict(count=count))):
                    got, cnt = ops.relation_reduce(op, t.t, gi, tt, n_rel, size, out_dtype=od, return_counts=True, **kw)
                    want, want_cnt = RR.relation_reduce_ref(op, t.values, sm, types, n_rel, dst_np, size)
                    assert same(torch, got, want) and np.array_equal(cnt.cpu().numpy(), want_cnt), (op, d, od, sorted(kw))
        assert big.count() == t.nnz


@pytest.mark.parametrize("d", bo.DIMS)
def test_sparse_feature_embedding(big, EA, O, d):
    """the embedding table is the big one; the uint64 feature values of a 24-node graph are the
    probe row numbers and values that name no row"""
    from test_sparse_embedding_gpu import chain_graph
    import feature_ref as FR
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(9400 + d)
    n_nodes = 24
    with big.table(d) as t:
        none = [t.rows, t.rows + 5, (1 << 33) + 5, (1 << 63) + 3]
        values = [int(x) for x in t.ids(rng, total=60)] + none
        values = [values[i] for i in rng.permutation(len(values))]
        cuts = np.sort(rng.integers(0, len(values) + 1, n_nodes - 1))
        cuts[5] = cuts[4]                                                         # a node without values
        lists = [np.array(v, np.uint64) for v in np.split(np.array(values, dtype=object), cuts)]
        small_lists = [np.array([int(t.compact([int(x)])[0]) if int(x) < t.rows else len(t.probe) + 7 for x in v],
                                np.uint64) for v in lists]
        node_ids = (np.arange(n_nodes, dtype=np.uint64) * 4 + 2)
        graph = chain_graph(EA, O, node_ids, sparse_features=FR.ragged_table([[v] for v in lists], np.uint64).as_tuple())
        try:
            q = torch.as_tensor(np.concatenate([node_ids, [3]]).astype(np.int64)).cuda()
            for combiner in SE.COMBINERS:
                want, _ = SE.embed(small_lists + [np.zeros(0, np.uint64)], None, t.values, combiner)
                for od in out_dtypes(torch, dt):
                    got, = graph.sparse_feature_embedding(q, [0], [t.t], combiner, [None], out_dtype=od)
                    assert same(torch, got, want), (d, combiner, od)
        finally:
            graph.close()
        assert big.count() == t.nnz


# ---- the whole table searched -------------------------------------------------------------------
QUERY_DT = {"f32": "bf16", "bf16": "f16", "f16": "f32"}                # the queries in a second dtype


# the four metrics at d = 136; ip and l2 (one per direction of the order) at d = 132 and 129: with all four
# there too these cases took 15.7 s a dtype on an MI355X, more than the module's other 16-bit cases together
SEARCH_CASES = [(metric, d) for d in bo.DIMS for metric in SR.METRICS if d == bo.DIMS[0] or metric in ("ip", "l2")]


@pytest.mark.parametrize("metric,d", SEARCH_CASES)
def test_table_search(big, ops, metric, d):
    """table_topk and table_rank over all 31.6 M rows: the offsets (int64_t)row * d + j * V of the
    scan, the slabs' lists at * k + lane and the merge's ((i / k) * q + qq) * k + i % k.  33 queries
    (two tiles): every probe row, a zero row, random rows in a second dtype.  k = 64 is more than
    the probe rows, so zero rows fill the tail of every list in row order - and precede the probe
    rows that score worse than a zero row.  Expected: table_search_ref.sparse_topk / sparse_rank on
    the small table (test_table_search_host.py holds them against the dense restatement).  This is the
    one shape that runs 512 slabs with every slab full-length: the cap and the long merge."""
    torch, dt = big.torch, big.dt
    dq, k = QUERY_DT[dt], bo.SEARCH_K
    rng = np.random.default_rng(9500 + d)
    with big.table(d) as t:
        q32, exclude, target = bo.search_case(rng, t.probe, t.values, bo.BIG, d, bo.ELEM_BYTES[dt])
        q32 = SR.to_dtype(q32, dq)
        assert np.array_equal(q32[:len(t.probe)], t.values) and len(q32) == bo.SEARCH_Q and len(t.probe) < k
        queries = dev(torch, store_ref.narrow(q32, dq), dq)
        # the launch shape, from the restatement: two tiles, the cap of 512 slabs, an item a block
        tiles = SR.tiles_of(len(q32), d)
        slabs = SR.slabs_of(t.rows, tiles)
        slab_rows = -(-t.rows // slabs)
        assert (tiles, slabs) == (2, SR.MAX_SLABS) and tiles * slabs <= SR.BLOCK_CAP
        assert (slabs - 1) * slab_rows < t.rows <= slabs * slab_rows and slab_rows > 60000
        v = SR.chunk_width(d, t.t.data_ptr(), t.t.element_size(), queries.data_ptr(), queries.element_size())
        assert v == (8 if d % 8 == 0 else 4 if d % 4 == 0 else 1)
        for exc in (None, exclude):
            got_s, got_r = ops.table_topk(t.t, queries, k, metric=metric, exclude=None if exc is None else dev(torch, exc))
            want_s, want_r = SR.sparse_topk(t.probe, t.values, t.rows, q32, k, metric, v, exc)
            assert np.all(want_r >= 0) and want_r.max() < t.rows
            assert SR.same_scores(got_s.cpu().numpy(), want_s), (metric, d, exc is None, "scores")
            assert np.array_equal(got_r.cpu().numpy(), want_r), (metric, d, exc is None, "rows")
            assert big.count() == t.nnz
        if metric == "l2":                                # once more with ids=: the second output is ids[rows]
            ids = torch.arange(t.rows, device="cuda") * 3 + 7
            got_s, got_r = ops.table_topk(t.t, queries, k, metric=metric, exclude=dev(torch, exclude), ids=ids)
            assert SR.same_scores(got_s.cpu().numpy(), want_s) and np.array_equal(got_r.cpu().numpy(), want_r * 3 + 7)
            del ids
            assert big.count() == t.nnz
        for exc in (None, exclude):
            got = ops.table_rank(t.t, queries, dev(torch, target), metric=metric,
                                 exclude=None if exc is None else dev(torch, exc))
            want = SR.sparse_rank(t.probe, t.values, t.rows, q32, target, metric, v, exc)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (metric, d, exc is None, "rank")
            assert big.count() == t.nnz
        assert want.min() == -1 and want.max() > t.rows - 2 * len(t.probe)


def kg_batch(t, rng, b=32, k=3, n_rel=7):
    """(src, rel_id, dst, neg) as numpy, and the same over the small table"""
    ids = t.ids(rng, extra=bo.no_row_ids(t.rows), total=b * (2 + k))
    src, dst, neg = ids[:b], ids[b:2 * b], ids[2 * b:].reshape(b, k)
    rel_id = rng.integers(0, n_rel, b)
    rel_id[[3, 9]] = [-1, n_rel + 2]
    return (src, rel_id, dst, neg), (t.compact(src), rel_id, t.compact(dst), t.compact(neg))


def kg_upstream(rng, want):
    return (rng.random(want[0].shape) * 8 - 4).astype(np.float32), (rng.random(want[1].shape) * 8 - 4).astype(np.float32)


@pytest.mark.parametrize("d", bo.DIMS)
@pytest.mark.parametrize("proj", ["hyperplane", "transfer"])
def test_triple_score_proj_sparse_grad(big, ops, proj, d):
    """TransH with ent the big table; TransD with ent the big table and ent_transfer a second table of
    its shape (its own allocation), both with sparse gradients over the probe rows"""
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(5100 + d)
    n_rel = 7
    n = bo.DIMS.index(d) + (proj == "transfer")
    kind, corrupt = TP.KINDS[n % 2], CORRUPTS[n % 3]
    with big.table(d) as t:
        ids, small = kg_batch(t, rng, n_rel=n_rel)
        rel32, rel_aux32 = bo.probe_values(rng, n_rel, d), bo.probe_values(rng, n_rel, d)
        rel, rel_aux = (dev(torch, store_ref.narrow(x, dt), dt) for x in (rel32, rel_aux32))
        ent = t.t.detach().requires_grad_()
        ent_aux32 = ent_aux = None
        if proj == "transfer":
            ent_aux32 = bo.probe_values(rng, len(t.probe), d)
            ent_aux = torch.zeros(t.t.shape, dtype=t.t.dtype, device="cuda")
            ent_aux[t.probe_t] = dev(torch, store_ref.narrow(ent_aux32, dt), dt)
            ent_aux.requires_grad_()
        v = TP.proj_chunk_width(d, ent.data_ptr(), 0 if ent_aux is None else ent_aux.data_ptr(), ent.element_size(),
                                rel.data_ptr(), rel_aux.data_ptr(), rel.element_size())
        kw = dict(hyper=rel_aux) if proj == "hyperplane" else dict(ent_transfer=ent_aux, rel_transfer=rel_aux)
        pos, out = ops.triple_score_proj(ent, rel, *[dev(torch, x) for x in ids], proj=proj, kind=kind, corrupt=corrupt,
                                         sparse_grad=True, **kw)
        want = TP.forward(proj, t.values, ent_aux32, rel32, rel_aux32, *small, kind, corrupt, v)
        assert np_same(pos, want[0]) and np_same(out, want[1]), (proj, kind, corrupt, d)
        g_pos, g_neg = kg_upstream(rng, want)
        ((pos * dev(torch, g_pos)).sum() + (out * dev(torch, g_neg)).sum()).backward()
        rows = TP.grad(proj, t.values, ent_aux32, rel32, rel_aux32, *small, kind, corrupt, v, g_pos, g_neg)
        keys = np.concatenate([ids[0], ids[2], ids[3].reshape(-1)])
        check_sparse_grad(torch, ent.grad, t, keys, np.concatenate([rows[0], rows[2], rows[3].reshape(-1, d)]))
        if proj == "transfer":
            check_sparse_grad(torch, ent_aux.grad, t, keys, np.concatenate([rows[5], rows[6], rows[7].reshape(-1, d)]))
            assert count_all(torch, ent_aux.detach()) == t.nnz
        del ent_aux
        assert big.count() == t.nnz


@pytest.mark.parametrize("d", bo.DIMS)
def test_triple_score_matrix_sparse_grad(big, ops, d):
    """TransR with ent [rows, de] the big table, dr = 12"""
    torch, dt = big.torch, big.dt
    rng = np.random.default_rng(5200 + d)
    n_rel, dr = 7, 12
    n = bo.DIMS.index(d)
    kind, corrupt = TM.KINDS[n % 2], CORRUPTS[(n + 1) % 3]
    with big.table(d) as t:
        ids, small = kg_batch(t, rng, n_rel=n_rel)
        rel32, matrix32 = bo.probe_values(rng, n_rel, dr), bo.probe_values(rng, n_rel, d * dr) / 16
        rel, matrix = (dev(torch, store_ref.narrow(x, dt), dt) for x in (rel32, matrix32))
        assert np.array_equal(store_ref.widen(store_ref.narrow(matrix32, dt), dt), matrix32)
        ent = t.t.detach().requires_grad_()
        v = TM.matrix_chunk_width(dr, rel.data_ptr(), rel.element_size())
        pos, out = ops.triple_score_matrix(ent, rel, matrix, *[dev(torch, x) for x in ids], kind=kind, corrupt=corrupt,
                                           sparse_grad=True)
        want = TM.forward(t.values, rel32, matrix32, *small, kind, corrupt, v)
        assert np_same(pos, want[0]) and np_same(out, want[1]), (kind, corrupt, d)
        g_pos, g_neg = kg_upstream(rng, want)
        ((pos * dev(torch, g_pos)).sum() + (out * dev(torch, g_neg)).sum()).backward()
        rows = TM.grad(t.values, rel32, matrix32, *small, kind, corrupt, v, g_pos, g_neg)
        check_sparse_grad(torch, ent.grad, t, np.concatenate([ids[0], ids[2], ids[3].reshape(-1)]),
                          np.concatenate([rows[0], rows[2], rows[3].reshape(-1, d)]))
        assert big.count() == t.nnz
