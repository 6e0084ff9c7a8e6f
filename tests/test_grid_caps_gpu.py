"""The fused ops PAST the grid caps of their launchers: every launcher in euler_amd/csrc clamps its
grid and lets the kernel loop, and these are the calls in which a block makes a second trip - a
stride with the wrong rows-per-block, per-trip state that is not reset (the scale cache of the fp8
gather, the `seen` counter and the masks of the long softmax kernels, the LDS slots and the tile of
the supervised loss) or a shuffle whose lanes leave the loop at different trips would show here
and nowhere else.  tests/grid_caps.py restates the grids and holds the cases;
test_grid_caps_host.py checks on the CPU that every case does pass its cap.

Expected values never come from the op under test: they are the numpy restatements of the ops
(mp_base_ref, weighted_mp_ref, fp8_ref, edge_softmax_ref, segment_attention_ref, supervise_ref,
relation_reduce_ref, gcn_norm_ref), compared bit for bit as each op's own test compares; edge_dot
keeps the float64 bound of test_weighted_mp_gpu.  The restatements of the reduces loop over the
destinations in Python, so - as test_mp_base_gpu.test_grid_stride_loops does - every destination
has 0, 1 or 2 updates, which makes the restated loop three vectorised steps (init, first update,
second update), a few long destinations placed in the first and in the last trip go through the
restatement itself, and so do probe rows at both ends and on either side of cap * rows-per-block.
Tables that are gathered from stay at a few hundred rows: only the destinations are many.

Left out, because a test already passes that cap with that kernel form: the fp32 plain reduces and
gather (test_mp_base_gpu.test_grid_stride_loops, test_gather_grid_stride_loop), the element forms
of relation_reduce and gcn_aggregate (their test_grid_stride / test_row_loop_strides_past_the_
block_cap), and TkGradKernel, whose grid TkBlocks caps at 2^20 blocks = 2^28 elements
(test_big_offsets_gpu.test_topk_gradient_past_2_32_selected_elements runs 2^32).  Also left out:
an attention call the short kernel does not serve (heads > 64) past the long grid's cap - 2^21
destinations x 65 heads is 136 M logits, and its restatement alone takes minutes."""
import functools

import numpy as np
import pytest
import torch

import dat_write
import edge_softmax_ref as SMX
import fp8_ref as F8
import gcn_norm_ref as GCN
import grid_caps as C
import mp_base_ref as B
import relation_reduce_ref as REL
import segment_attention_ref as ATT
import supervise_ref as SV
import weighted_mp_ref as WR
from test_fp8_rows_gpu import make_table, xhat_cpu
from test_segment_attention_gpu import Block as AttBlock
from test_supervise_gpu import check as sv_check, raw as sv_raw
from test_weighted_mp_gpu import dot_bound, within

pytestmark = pytest.mark.gpu

F = np.float32
F32 = torch.float32
S16 = {"bf16": torch.bfloat16, "f16": torch.float16}
MODES = ("add", "max", "mean")
ROWS = 300


@pytest.fixture(scope="module")
def ops(EA):
    return EA.ops


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def same(got, want):
    """the dtype, the shape and the bits of want (a tensor, or an array that is uploaded first)"""
    if isinstance(want, np.ndarray):
        want = dev(want)
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(bits(got), bits(want.to(got.device)))


def rounded(want32, S):
    """ONE rounding of an fp32 result to a 16-bit dtype, by torch on the CPU"""
    return torch.from_numpy(np.ascontiguousarray(want32, F)).to(S)


def table16(shape, S, seed, scale=8.0):
    """values of dtype S in [-scale / 2, scale / 2] -> (the table on the device, its values as float32)"""
    rng = np.random.default_rng(seed)
    t = torch.from_numpy(((rng.random(shape) - 0.5) * scale).astype(F)).to(S)
    return t.cuda(), t.float().numpy()


def table32(shape, seed):
    """fp32 values over six decades: a sum in another order has other bits"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(F)
    return dev(x), x


def stable_shuffle(keys, seed):
    """slot j of the shuffled block holds grouped update perm[j]: unsorted keys whose stable sort
    restores the grouped order (the order INSIDE a destination is kept)"""
    e = len(keys)
    slot_keys = keys[np.random.default_rng(seed).permutation(e)]
    perm = np.empty(e, np.int64)
    perm[np.argsort(slot_keys, kind="stable")] = np.arange(e)
    return perm


def probe_rows(grid, size):
    """both ends, and either side of the first item that only a second trip writes"""
    edge = grid.first_trip
    assert grid.strides and 3 <= edge < size
    return sorted(r for r in {0, 1, 2, edge - 2, edge - 1, edge, edge + 1, size - 3, size - 2, size - 1} if r < size)


# ---- the reduces: 16-bit, fp32 weighted, fp8 ------------------------------------------------------
class Updates(object):
    """`size` destinations of 0, 1 or 2 updates, two long ones (37 in the first trip, 21 in the last),
    gather rows into a table of `rows` rows, sorted keys, the stable shuffle, int64 ids whose high
    word is set here and there (only the low word counts); and a second block of `count` = 2"""

    def __init__(self, size, rows):
        self.size = size
        self.lens = C.seg_lengths(size, size + rows, long_at=(5, size - 6), long_len=(37, 21))
        self.ptr = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.e = int(self.ptr[-1])
        rng = np.random.default_rng(size + 7 * rows)
        self.gi = rng.integers(0, rows, self.e).astype(np.int32)
        self.keys = np.repeat(np.arange(size, dtype=np.int32), self.lens)
        self.perm = stable_shuffle(self.keys, size)
        ids = self.gi.astype(np.int64)
        ids[::7] += 1 << 33
        self.gi2 = rng.integers(0, rows, 2 * size).astype(np.int32)
        self.ptr2 = np.arange(size + 1, dtype=np.int64) * 2
        self.d = {k: dev(v) for k, v in dict(gi=self.gi, keys=self.keys, ptr=self.ptr, ids=ids, gi2=self.gi2,
                                              perm=self.perm, gi_p=self.gi[self.perm],
                                              keys_p=self.keys[self.perm]).items()}


@functools.lru_cache(maxsize=2)
def updates(size, rows):
    return Updates(size, rows)


def one_row(op, x, gi, ptr, w, r):
    """destination r by the op's restatement: the Python loop over its updates in input order"""
    b, en = int(ptr[r]), int(ptr[r + 1])
    if w is None:
        return B.reduce_rows(op, x[gi[b:en]], x.shape[1])
    return WR.reduce_segment(op, x, w, gi[b:en], np.arange(b, en))


def reduce_expected(op, x, gi, ptr, w=None):
    """The restated loop of mp_base_ref.reduce_rows / weighted_mp_ref.reduce_segment for segments
    of at most two updates, a step at a time and every destination at once: acc = init; acc = acc (+ or
    max) m0; acc = acc (+ or max) m1, m = the gathered row (times its edge's weights, one rounding);
    the mean's one division.  Longer segments go through the restatement itself."""
    lens = np.diff(ptr)
    e, d = len(gi), x.shape[1]

    def message(p):
        m = x[gi[p]]
        return m if w is None else (m * np.repeat(w[p], d // w.shape[1], axis=1)).astype(F)
    n = lens[:, None]
    m0 = message(np.minimum(ptr[:-1], e - 1))
    m1 = message(np.minimum(ptr[:-1] + 1, e - 1))
    init = F(B.INIT[op])
    if op == "max":
        a1 = np.where(m0 > init, m0, init)
        a2 = np.where(m1 > a1, m1, a1)
    else:
        a1 = init + m0
        a2 = a1 + m1
    out = np.where(n == 0, init, np.where(n == 1, a1, a2)).astype(F)
    if op == "mean":
        out = (out / B.mean_denominator(lens)[:, None]).astype(F)
    for r in np.flatnonzero(lens > 2):
        out[r] = one_row(op, x, gi, ptr, w, r)
    return out


def weights(e, heads, WS, seed):
    """edge weights of dtype WS in [-2, 2] without zeros -> (on the device, as float32)"""
    rng = np.random.default_rng(seed)
    w = ((rng.random((e, heads)) - 0.5) * 4).astype(F)
    w[np.abs(w) < 0.01] = 1
    t = torch.from_numpy(w).to(WS)
    return t.cuda(), t.float().numpy()


def check_reduces(ops, t, x, size, grid, heads=0, w_dtypes=(F32,), out16=None, keyed=True):
    """Every mode through every destination form on table t (a tensor, or an Fp8Rows; x: its values
    as float32): seg_ptr with int32 rows and with int64 ids, sorted keys, shuffled keys (the perm
    path), count; fp32 out everywhere, a 16-bit out through seg_ptr and sorted keys."""
    rows, d = x.shape
    u = updates(size, rows)
    g = u.d
    probes = probe_rows(grid, size)
    assert u.lens[probes[-1]] > 0 and u.lens[size - 6] > 2 and size - 6 >= grid.first_trip
    for wi, WS in enumerate(w_dtypes if heads else (None,)):
        w_dev = w = w2_dev = w2 = None
        if heads:
            w_dev, w = weights(u.e, heads, WS, size + heads)
            w2_dev, w2 = weights(2 * size, heads, WS, size + heads + 1)
        kw = {} if w is None else dict(edge_weight=w_dev)
        kw_p = {} if w is None else dict(edge_weight=w_dev[g["perm"]].contiguous())
        kw2 = {} if w is None else dict(edge_weight=w2_dev)
        for op in (MODES if wi == 0 else ("max", "mean")):
            want = reduce_expected(op, x, u.gi, u.ptr, w)
            for r in probes:
                assert np.array_equal(want[r].view(np.uint32), one_row(op, x, u.gi, u.ptr, w, r).view(np.uint32)), r
            want_dev = dev(want)
            got = {"seg_ptr": ops.gather_segment_reduce(op, t, g["gi"], size, seg_ptr=g["ptr"], out_dtype=F32, **kw),
                   "ids": ops.gather_segment_reduce(op, t, g["ids"], size, seg_ptr=g["ptr"], out_dtype=F32, **kw)}
            if keyed:
                got["sorted"] = ops.gather_scatter(op, t, g["gi"], g["keys"], size, out_dtype=F32, **kw)
                got["shuffled"] = ops.gather_scatter(op, t, g["gi_p"], g["keys_p"], size, out_dtype=F32, **kw_p)
            for form, out in got.items():
                assert same(out, want_dev), (op, form, WS)
            if out16 is not None:
                want16 = rounded(want, out16).cuda()
                assert same(ops.gather_segment_reduce(op, t, g["gi"], size, seg_ptr=g["ptr"], out_dtype=out16, **kw),
                            want16), (op, "seg_ptr", out16)
                if keyed:
                    assert same(ops.gather_scatter(op, t, g["gi"], g["keys"], size, out_dtype=out16, **kw),
                                want16), (op, "sorted", out16)
            want = reduce_expected(op, x, u.gi2, u.ptr2, w2)
            for r in probes:
                assert np.array_equal(want[r].view(np.uint32), one_row(op, x, u.gi2, u.ptr2, w2, r).view(np.uint32)), r
            assert same(ops.gather_segment_reduce(op, t, g["gi2"], size, count=2, out_dtype=F32, **kw2), want), \
                (op, "count", WS)
            if out16 is not None:
                assert same(ops.gather_segment_reduce(op, t, g["gi2"], size, count=2, out_dtype=out16, **kw2),
                            rounded(want, out16)), (op, "count", out16)


@pytest.mark.parametrize("which", ["bf16", "f16"])
@pytest.mark.parametrize("d,size", C.HALF_PLAIN)
def test_half_reduces(ops, which, d, size):
    """SegmentReduceHalfKernel (d = 3) and SegmentReduceVec8Kernel with 4 (d = 512) and 256 (d = 8)
    rows a block"""
    S = S16[which]
    t, x = table16((ROWS, d), S, d)
    check_reduces(ops, t, x, size, C.row_lane_shape(size, d, 8), out16=S)


@pytest.mark.parametrize("which", ["bf16", "f16"])
@pytest.mark.parametrize("d,heads,size", C.HALF_WEIGHTED)
def test_half_weighted_reduces(ops, which, d, heads, size):
    """the vector form (dh = 128) and the element form (dh = 4 is no multiple of 8); weights in fp32
    and in the table's dtype"""
    S = S16[which]
    t, x = table16((ROWS, d), S, d + heads)
    check_reduces(ops, t, x, size, C.row_lane_shape(size, d, 8, d // heads), heads=heads, w_dtypes=(F32, S), out16=S)


@pytest.mark.parametrize("d,heads,size", C.F32_WEIGHTED)
def test_f32_weighted_reduces(ops, d, heads, size):
    """LaunchWeightedReduce: the element form (d = 3; d = 8 with dh = 2) and Vec4 with 4 and 256 rows a block"""
    t, x = table32((ROWS, d), d + heads)
    check_reduces(ops, t, x, size, C.row_lane_shape(size, d, 4, d // heads), heads=heads)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("d,size,out", C.FP8_REDUCE)
def test_fp8_reduces(EA, ops, d, size, out, weighted):
    """the element kernels (d = 3) and the Vec16 ones with 4 (d = 1024) and 256 (d = 16) rows a block"""
    q, scale = make_table(np.random.default_rng(d), ROWS, d)
    x = xhat_cpu(torch, q, scale)
    T = EA.ops.Fp8Rows(dev(q), dev(scale))
    heads = 1 if weighted else 0
    check_reduces(ops, T, x, size, C.row_lane_shape(size, d, 16, d if weighted else 0), heads=heads,
                  w_dtypes=(F32, torch.bfloat16), out16=torch.bfloat16 if out == "bf16" else torch.float16, keyed=False)


# ---- fp8: gather, quantise, column absmax ---------------------------------------------------------
@pytest.mark.parametrize("d,e,out16,cache_stays", C.FP8_GATHER)
def test_fp8_gather(EA, ops, d, e, out16, cache_stays):
    """Fp8GatherKernel past 2^20 lanes: the scale cache of a lane reloads on every trip (dv = 3 does
    not divide the stride), stays (dv = 4), the 16-code lanes to bf16, the element form"""
    grid, dv = C.fp8_gather_grid(e, d, out16)
    assert grid.strides and (cache_stays is None or (grid.first_trip % dv == 0) == cache_stays)
    rng = np.random.default_rng(e + d)
    q, scale = make_table(rng, 1000, d)
    x = xhat_cpu(torch, q, scale)
    idx = rng.integers(0, 1000, e).astype(np.int32)
    idx[-3:] = [999, 0, 500]
    T = EA.ops.Fp8Rows(dev(q), dev(scale))
    want = F8.dequantize(q, scale)[idx]
    assert np.array_equal(want.view(np.uint32), x[idx].view(np.uint32))
    got = ops.gather(T, dev(idx), out_dtype=torch.bfloat16 if out16 else None)
    assert same(got, rounded(want, torch.bfloat16) if out16 else want)


@pytest.mark.parametrize("src", ["float32", "bfloat16"])
def test_fp8_quantize(EA, ops, src):
    n, d = C.FP8_QUANTIZE
    assert C.grid_for(n * d).strides
    rng = np.random.default_rng(n)
    x = torch.from_numpy((rng.standard_normal((n, d)) * np.exp2(rng.integers(-6, 6, (n, d)))).astype(F))
    x = x.to(getattr(torch, src))
    scale = (rng.uniform(0.5, 1.0, d) * 0.037).astype(F)
    T = EA.ops.Fp8Rows.quantize(x.cuda(), dev(scale))
    want = F8.quantize(x.float().numpy(), scale)
    assert len(np.unique(want[-1000:])) > 50
    assert same(T.q, want)


@pytest.mark.parametrize("n,d", C.FP8_ABSMAX)
def test_fp8_column_absmax(ops, n, d):
    """the largest value of some columns lies in rows that only a second trip of the row loop reads"""
    grid, by = C.column_absmax_grid(n, d)
    assert grid.strides
    rng = np.random.default_rng(n + d)
    x = rng.standard_normal((n, d)).astype(F)
    x[n - 1, 1::4] = 77.5
    x[grid.first_trip + 3, d - 1] = -99.25
    want = F8.column_absmax(x)
    assert want[d - 1] == F(99.25) and (want[1::4][:-1] == F(77.5)).all() and want[1] == F(77.5)
    assert same(ops.column_absmax(dev(x)), want)
    xs = torch.from_numpy(x).to(torch.bfloat16)
    assert same(ops.column_absmax(xs.cuda()), F8.column_absmax(xs.float().numpy()))


# ---- edge_dot ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,heads,e", C.EDGE_DOT)
def test_edge_dot(ops, d, heads, e):
    """64 lanes a task (d = 512), V = 4 with three chunks on four lanes (dh = 12), a lane a task (d = 1);
    the bound of test_weighted_mp_gpu, and the last tasks - a second trip - alone give the same bits"""
    grid, v, log_l = C.edge_dot_grid(e, heads, d)
    assert grid.strides
    gen = torch.Generator(device="cuda")
    gen.manual_seed(e)
    ra, rb = 150, 170
    ai = torch.randint(0, ra, (e,), generator=gen, device="cuda", dtype=torch.int32)
    bi = torch.randint(0, rb, (e,), generator=gen, device="cuda", dtype=torch.int32)
    for SA, SB in ((F32, F32), (torch.bfloat16, torch.bfloat16)):
        a = ((torch.rand((ra, d), generator=gen, device="cuda") - 0.5) * 8).to(SA)
        b = ((torch.rand((rb, d), generator=gen, device="cuda") - 0.5) * 8).to(SB)
        a_rows, b_rows = a.float()[ai.long()], b.float()[bi.long()]
        for od in {F32, SA}:
            got = ops.edge_dot(a, ai, b, bi, heads=heads, out_dtype=od)
            assert got.shape == (e, heads) and got.dtype == od
            want, bound = dot_bound(torch, a_rows, b_rows, heads, od)
            assert within(torch, got, want, bound), (SA, od)
            assert same(got[-37:], ops.edge_dot(a, ai[-37:], b, bi[-37:], heads=heads, out_dtype=od))
            if d == heads:        # one product a task: exact
                assert same(got, (a_rows * b_rows).to(od))
        # no index arrays: task p reads row p of both
        ar, br = a[ai.long()].contiguous(), b[bi.long()].contiguous()
        assert same(ops.edge_dot(ar, None, br, None, heads=heads, out_dtype=F32),
                    ops.edge_dot(a, ai, b, bi, heads=heads, out_dtype=F32))
        del ar, br, a_rows, b_rows


# ---- edge_softmax -----------------------------------------------------------------------------------
def smx_logits(rng, e, heads):
    x = (rng.standard_normal((e, heads)) * 4).astype(F)
    x[rng.random(e) < 0.01] -= F(100.0)           # differences to the maximum beyond the floor: flushed
    return x


def smx_forms(ops, x, g, lens, size, count=None, seed=0):
    """The forward on x, then the raw gradient entry on (y, g), through seg_ptr, sorted keys,
    shuffled keys and (uniform blocks) count -> (y, gx), after asserting that the forms agree"""
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keys = np.repeat(np.arange(size, dtype=np.int32), lens)
    perm = dev(stable_shuffle(keys, seed))
    sp, k = dev(ptr), dev(keys)
    kp = k[perm].contiguous()
    od = x.dtype

    def every(a, b):
        outs = [ops._edge_softmax_raw(a, b, None, sp, 0, size, od), ops._edge_softmax_raw(a, b, k, None, 0, size, od)]
        if count is not None:
            outs.append(ops._edge_softmax_raw(a, b, None, None, count, size, od))
        shuffled = ops._edge_softmax_raw(a[perm].contiguous(), None if b is None else b[perm].contiguous(), kp, None,
                                         0, size, od)
        back = torch.empty_like(shuffled)
        back[perm] = shuffled
        for o in outs[1:] + [back]:
            assert same(o, outs[0])
        return outs[0]
    y = every(x, None)
    assert same(ops.edge_softmax(x, seg_ptr=sp), y)
    return y, every(y, g)


def test_edge_softmax_short_kernel_uniform(ops):
    """the K = 16 kernel past 2 097 152 (destination, head) tasks"""
    size, heads, count = C.SMX_SHORT_SIZE, C.SMX_SHORT_HEADS, 2
    assert C.smx_short_grid(size, heads).strides
    rng = np.random.default_rng(1)
    x_np, g_np = smx_logits(rng, size * count, heads), rng.standard_normal((size * count, heads)).astype(F)
    ptr = np.arange(size + 1, dtype=np.int64) * count
    want = SMX.edge_softmax_ref(x_np, ptr)
    y, gx = smx_forms(ops, dev(x_np), dev(g_np), np.full(size, count), size, count=count)
    assert same(y, want)
    assert same(gx, SMX.edge_softmax_ref(want, ptr, g_np))


def test_edge_softmax_short_and_long_kernels_ragged(ops):
    """the K = 32 kernel past its cap and the long kernel (share 1) on the same call: lengths 0 .. 3
    and a few segments of 33 and 300 updates at both ends"""
    size, heads = C.SMX_SHORT_SIZE, C.SMX_SHORT_HEADS
    at, n = C.smx_long_segments(size)
    lens = C.seg_lengths(size, 2, at, n, high=4)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    e = int(ptr[-1])
    rng = np.random.default_rng(2)
    x_np, g_np = smx_logits(rng, e, heads), rng.standard_normal((e, heads)).astype(F)
    want = SMX.edge_softmax_ref(x_np, ptr)
    y, gx = smx_forms(ops, dev(x_np), dev(g_np), lens, size)
    assert same(y, want)
    assert same(gx, SMX.edge_softmax_ref(want, ptr, g_np))


def test_edge_softmax_zero_fill_loop(ops):
    """300 000 updates whose key names no destination, 8 heads: more (update, head) pairs than the
    full short grid has lanes, into memory that held something else"""
    outside, heads, size = C.SMX_FILL
    assert C.smx_zero_fill_grid(outside, heads, size).strides
    lens = C.seg_lengths(size, 3)
    rng = np.random.default_rng(3)
    inside = np.repeat(np.arange(size, dtype=np.int32), lens)
    keys = np.concatenate([np.full(700, -2, np.int32), inside, size + rng.integers(0, 9, outside - 700).astype(np.int32)])
    keys.sort()
    e = len(keys)
    ptr = SMX.seg_ptr_of_sorted_keys(keys, size)
    x_np, g_np = smx_logits(rng, e, heads), rng.standard_normal((e, heads)).astype(F)
    want = SMX.edge_softmax_ref(x_np, ptr)
    want_g = SMX.edge_softmax_ref(want, ptr, g_np)
    assert not want[:700].any() and not want[-(outside - 700):].any() and want[700:-(outside - 700)].any()
    perm = stable_shuffle(keys, 3)
    for order in (None, perm):
        x, g, k = (dev(a if order is None else a[order]) for a in (x_np, g_np, keys))
        for S in (F32, torch.bfloat16):
            dirty = torch.full((e, heads), 7.0, device="cuda", dtype=S)
            del dirty                                 # (the allocator hands it to the next output)
            y = ops.edge_softmax(x.to(S), indices=k, size=size, out_dtype=F32)
            if S == F32:
                assert same(y, want if order is None else want[order])
                dirty = torch.full((e, heads), 7.0, device="cuda")
                del dirty
                gx = ops._edge_softmax_raw(y, g, k, None, 0, size, F32)
                assert same(gx, want_g if order is None else want_g[order])
            outsider = (k < 0) | (k >= size)
            assert not bool(y[outsider].any()) and int(outsider.sum()) == outside


@pytest.mark.parametrize("heads", C.SMX_LONG_HEADS)
@pytest.mark.parametrize("size,share", C.SMX_LONG)
def test_edge_softmax_long_kernel(ops, size, share, heads):
    """EdgeSoftmaxLongKernel with a share between its extremes (13, 3), share 1 without a stride, and
    strided chunks; long segments among the first 300 and the last 300 destinations, several in one
    chunk so that the blocks of a chunk split them; a head at a time (1, 3) and all heads at once (8)"""
    grid, claimed = C.smx_long_grid(size)
    assert claimed == share
    at, n = C.smx_long_segments(size)
    lens = C.seg_lengths(size, size, at, n)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    e = int(ptr[-1])
    rng = np.random.default_rng(size + heads)
    x_np, g_np = smx_logits(rng, e, heads), rng.standard_normal((e, heads)).astype(F)
    want = SMX.edge_softmax_ref(x_np, ptr)
    y, gx = smx_forms(ops, dev(x_np), dev(g_np), lens, size, seed=heads)
    assert same(y, want)
    assert same(gx, SMX.edge_softmax_ref(want, ptr, g_np))
    if heads == 3:         # 16-bit storage: the fp32 op on the widened logits, rounded once
        xs = torch.from_numpy(x_np).to(torch.bfloat16)
        want16 = SMX.edge_softmax_ref(xs.float().numpy(), ptr)
        assert same(ops.edge_softmax(xs.cuda(), seg_ptr=dev(ptr)), rounded(want16, torch.bfloat16))
        assert same(ops.edge_softmax(xs.cuda(), seg_ptr=dev(ptr), out_dtype=F32), want16)


# ---- attention_aggregate ----------------------------------------------------------------------------
def att_check(ops, b, forms):
    """forward (out, alpha, logits) and the destination side of the backward against the restatement"""
    x, alpha, out = b.want()
    q = torch.as_tensor(b.q, device="cuda").requires_grad_()
    got, a, lg = b.call(ops, q=q, return_attention=True, return_logits=True, **forms[0])
    assert same(lg, x), "logits"
    assert same(a, alpha), "alpha"
    assert same(got.detach(), out), "out"
    for form in forms[1:]:
        again, a2 = b.call(ops, return_attention=True, **form)
        assert same(again, got.detach()) and same(a2, a), sorted(form)
    got.backward(dev(b.grad))
    ds, dq = ATT.backward(b.kind, b.q, b.k, b.v, b.gi, b.sp, b.heads, alpha, b.grad, scale=b.scale, slope=b.slope)
    assert same(q.grad, dq), "grad_q"


@pytest.mark.parametrize("d,size,count", C.ATT_SHORT)
def test_attention_short_kernel(ops, d, size, count):
    """SegAttShortKernel past 16 384 blocks: 64 lanes a destination (d = 256: four a block) and one
    (d = 1: 256 a block); forward and backward"""
    for grad in (False, True):
        grid, log_g = C.att_short_grid(size, 1, d, d, "dot", grad)
        assert grid.strides
    b = AttBlock("dot", 1, d, [count] * size, shared=(d == 1), rows=ROWS, seed=size)
    att_check(ops, b, [dict(count=count), dict(seg_ptr=dev(b.sp)), dict(indices=dev(b.keys))])


@pytest.mark.parametrize("kind", ["dot", "additive"])
@pytest.mark.parametrize("size", C.ATT_LONG)
def test_attention_long_kernel(ops, kind, size):
    """SegAttLongKernel beside the short one on mixed segments, d = 1: share 13, and strided chunks"""
    at, n = C.smx_long_segments(size)
    lens = C.seg_lengths(size, size + 1, at, n)
    b = AttBlock(kind, 1, 1, lens, rows=ROWS, seed=size)
    att_check(ops, b, [dict(seg_ptr=dev(b.sp)), dict(indices=dev(b.keys))])


# ---- supervise_loss ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def sv_case(b, c):
    """inputs and the restatement without a histogram: shared by the cases of one shape"""
    x, z = C.supervise_inputs(b, c)
    want = SV.forward(x, z)
    for a in (x, z) + tuple(v for v in want.values() if isinstance(v, np.ndarray)):
        a.flags.writeable = False
    return x, z, want


def sv_want(b, c, t):
    x, z, want = sv_case(b, c)
    want = dict(want)
    if t is not None:
        want["hist"] = SV.hist_of(want["prob"], z, t)
    return x, z, want


def sv_run(EA, x, z, want, t, tag):
    from euler_amd import metrics
    ops = EA.ops
    xd, zd = dev(x), dev(z)
    sv_check(torch, sv_raw(torch, xd, zd, t), want, tag, t)
    metric = None if t is None else metrics.Streaming("auc", num_thresholds=t, device="cuda")
    loss, prob = ops.supervise_loss(xd, zd, metric=metric, return_prob=True)
    assert same(loss.reshape(1), np.array([want["loss"]], F)) and same(prob, want["prob"])
    if t is not None:
        assert np.array_equal(metric.counts.cpu().numpy(), want["counts"])
        assert np.array_equal(metric.hist.cpu().numpy(), want["hist"])
    b, c = x.shape
    g = 1.5
    got = ops._supervise_loss_grad_raw(dev(want["diff"]), torch.tensor(g, device="cuda"), F32)
    assert same(got, SV.grad(want["diff"], g, b, c))


@pytest.mark.parametrize("mode,t,c,b", C.SUPERVISE)
def test_supervise_loss_tile_loop(EA, mode, t, c, b):
    """SuperviseLossKernel past its 512 (LDS histogram) and 4096 tiles, both tile shapes, all three
    histogram modes; the raw entry, ops.supervise_loss and the gradient entry"""
    grid, claimed = C.supervise_grid(b, c, t)
    assert grid.strides and claimed == mode
    x, z, want = sv_want(b, c, t)
    sv_run(EA, x, z, want, t, (mode, c, b))


@pytest.mark.parametrize("b,c,t,mode", C.SUPERVISE_LIMIT)
def test_supervise_loss_histogram_limit(EA, b, c, t, mode):
    """T = 5719 asks for exactly 64 KiB of dynamic LDS - the last launch with the histogram in LDS -,
    5720 is the first with the histogram in memory, 20 000 a large one"""
    assert C.supervise_mode(t) == mode
    x, z, want = sv_want(b, c, t)
    sv_run(EA, x, z, want, t, (mode, c, b, t))


def test_supervise_loss_graph_form(EA, tmp_path):
    """the labels read from a graph's dense feature, past the 512-tile cap: 40 nodes, 131 329 queries"""
    mode, t, c, b = C.SUPERVISE_GRAPH
    grid, claimed = C.supervise_grid(b, c, t)
    assert grid.strides and claimed == mode
    rng = np.random.default_rng(5)
    ids = np.arange(40) * 3 + 5
    floats = []
    for i in range(40):
        hard = (rng.random(c) < 0.5).astype(F)
        hard[i % c] = rng.integers(0, 9) / 8.0
        floats.append([rng.normal(size=5).astype(F), hard[:1 + i % 3], hard])
    dat_write.write_feature_dat_dir(tmp_path, ids, floats, partitions=2)
    G = EA.Graph.load(str(tmp_path))
    q = rng.choice(ids, b).astype(np.int64)
    q[::1001] = 987654321                                  # unknown ids: labels 0
    nodes = dev(q)
    x, _ = C.supervise_inputs(b, c)
    xd = dev(x)
    for fid in (2, 1):                                     # the whole slot, and one shorter than c
        rows = G.get_dense_feature(nodes, [fid], [c])[0]
        z = rows.float().cpu().numpy()
        assert z[-300:].any() and (z[-300:] == 0).any()
        want = SV.forward(x, z, t)
        sv_check(torch, sv_raw(torch, xd, None, t, graph=G, nodes=nodes, fid=fid), want, ("graph", fid), t)


# ---- relation_reduce and gcn_aggregate, vector forms -----------------------------------------------
def relation_expected(op, x, gi, types, R):
    """relation_reduce_ref.reduce_dest for two updates a destination, every destination at once"""
    size = len(gi) // 2
    g, t = gi.reshape(size, 2), types.reshape(size, 2)
    valid = ((t >= 0) & (t < R)).sum(1)
    out = np.empty((size, R, x.shape[1]), F)
    cnt = np.zeros((size, R), np.int32)
    for rel in range(R):
        acc = np.full((size, x.shape[1]), REL.EMPTY["max"] if op == "max" else 0.0, F)
        for j in range(2):
            hit = (t[:, j] == rel)[:, None]
            v = x[g[:, j]]
            acc = np.where(hit, np.where(v > acc, v, acc) if op == "max" else acc + v, acc)
            cnt[:, rel] += t[:, j] == rel
        if op == "mean":
            acc = acc / (valid.astype(F) + F(1e-7))[:, None]
        elif op == "mean_rel":
            acc = acc / (cnt[:, rel].astype(F) + F(1e-7))[:, None]
        out[:, rel] = acc
    return out, cnt


@pytest.mark.parametrize("dtype,d,size,R", C.RELATION_VEC)
def test_relation_reduce_vector_form(ops, dtype, d, size, R):
    """RelationReduceVecKernel with four destinations a block, past 8192 blocks"""
    grid = C.row_lane_shape(size, d, C.LANE_N[dtype])
    assert C.row_lane_vec(d, C.LANE_N[dtype])
    rng = np.random.default_rng(size + d)
    S = F32 if dtype == "f32" else S16[dtype]
    t, x = table32((ROWS, d), d) if dtype == "f32" else table16((ROWS, d), S, d)
    gi = rng.integers(0, ROWS, 2 * size).astype(np.int32)
    types = rng.integers(-1, R + 1, 2 * size).astype(np.int32)      # -1 and R: left out
    types[-2:] = [0, R - 1]
    gd, td = dev(gi), dev(types)
    for op in REL.OPS:
        want, cnt = relation_expected(op, x, gi, types, R)
        for r in probe_rows(grid, size):
            one, c1 = REL.reduce_dest(op, x, gi[2 * r:2 * r + 2], types[2 * r:2 * r + 2], R)
            assert np.array_equal(want[r].view(np.uint32), one.view(np.uint32)) and np.array_equal(cnt[r], c1)
        got, counts = ops.relation_reduce(op, t, gd, td, R, size, count=2, out_dtype=F32, return_counts=True)
        assert same(got, want), op
        assert np.array_equal(counts.cpu().numpy(), cnt), op
        keys = dev(np.repeat(np.arange(size, dtype=np.int32), 2))
        assert same(ops.relation_reduce(op, t, gd, td, R, size, indices=keys, out_dtype=F32), got), op
        if S != F32:
            assert same(ops.relation_reduce(op, t, gd, td, R, size, count=2), rounded(want, S)), op


def test_gcn_aggregate_vector_form(ops):
    """gather_reduce_norm's vector form (d = 256: four rows a block) with a root term, one row past 8192
    blocks: that row, the only one of a second trip, has eleven updates"""
    d, size = C.GCN_VEC
    grid = C.row_lane_shape(size, d, 4)
    lens = C.seg_lengths(size, size, long_at=(5, size - 1), long_len=(19, 11))
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rng = np.random.default_rng(size)
    src = rng.integers(0, ROWS, int(ptr[-1])).astype(np.int32)
    dst = np.repeat(np.arange(size), lens)
    t, x = table32((ROWS, d), d)
    root_dev, root = table32((size, d), d + 1)
    nd, ns = GCN.gcn_norm(dst, src, size, ROWS)
    # the restated loop, a step at a time: w = fl(nd * ns[g]), m = fl(x[g] * w), acc = fl(acc + m)
    e = len(src)

    def message(p):
        return (x[src[p]] * (nd * ns[src[p]]).astype(F)[:, None]).astype(F)
    a1 = F(0) + message(np.minimum(ptr[:-1], e - 1))
    a2 = a1 + message(np.minimum(ptr[:-1] + 1, e - 1))
    n = lens[:, None]
    for op in ("add", "mean"):
        agg = np.where(n == 0, F(0), np.where(n == 1, a1, a2)).astype(F)
        if op == "mean":
            agg = (agg / (lens.astype(F) + F(1e-7))[:, None]).astype(F)
        for r in sorted(set(probe_rows(grid, size)) | set(np.flatnonzero(lens > 2).tolist())):
            one = GCN.reduce_segment(op, x, src[ptr[r]:ptr[r + 1]], nd[r], ns)
            if lens[r] > 2:
                agg[r] = one
            assert np.array_equal(agg[r].view(np.uint32), one.view(np.uint32)), r
        want = GCN.epilogue(agg, root, 0.75, 0.25)
        norm = (dev(nd), dev(ns))
        got = ops.gcn_aggregate(t, dev(src), (size, ROWS), norm, op=op, root=root_dev, alpha=0.25, seg_ptr=dev(ptr))
        assert same(got, want), op
        edges = (dev(dst.astype(np.int32)), dev(src))
        assert same(ops.gcn_aggregate(t, edges, (size, ROWS), norm, op=op, root=root_dev, alpha=0.25), got), op


# ---- gather_segment_topk ---------------------------------------------------------------------------
def test_gather_segment_topk_past_2_28_lanes(ops):
    """TkKernel past 2^20 blocks: bf16, d = 1, k = 1, count = 1 - out is the gathered element, sel the
    position.  About 3 GiB of device memory."""
    size = C.TOPK_SIZE
    assert C.tk_grid(size).strides
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory, %.1f GiB are free" % (free / 2.0 ** 30))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(28)
    table = ((torch.rand((50, 1), generator=gen, device="cuda") - 0.5) * 8).to(torch.bfloat16)
    gi = torch.randint(0, 50, (size,), generator=gen, device="cuda", dtype=torch.int32)
    out, sel = ops.gather_segment_topk(table, gi, size, 1, count=1, return_indices=True)
    assert out.shape == (size, 1, 1) and sel.shape == (size, 1, 1) and out.dtype == torch.bfloat16
    assert torch.equal(bits(out).view(-1), bits(table).view(-1)[gi.long()])
    del out
    assert torch.equal(sel.view(-1), torch.arange(size, device="cuda", dtype=torch.int32))
