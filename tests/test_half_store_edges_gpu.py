"""Every op's own 16-bit store rounds ONCE at the rounding edges of its storage type.

For an op f with inputs of dtype S (bf16, fp16), the test is

    bits of f(x, out_dtype=S)  ==  round_cpu(f(x, out_dtype=float32), S)

with torch's CPU conversion on the right (tests/half_edges.py) and the NaN rule of that file.  What
f computes in fp32 is the business of the op's own test file; what those files never reach are
fp32 results in S's subnormal range, beyond its largest finite value, and infinities and NaNs.

Inputs are 16-bit values +- m * 2^k, one table row per edge.  The binade k follows the edge's
DESTINATION: a third of the destinations sit around S's subnormal range, a third around 1, a third
just below S's largest finite value, so that sums, products and means land where the store has to
produce subnormals and infinities.  Because a bf16 result rounds to inf only from the last 1 / 512
of fp32's top binade, a few destinations are built to land there (the `top` destinations of Block):
  T1  one edge: the second-largest S value (times a weight 1 + ulp where the op has weights, or
      plus a root row of 3.5 half-units);
  T2  two edges: the largest S value and 1.1 .. 1.9 half-units of its last place, same sign;
  T4  four edges: largest, largest, 2.2 .. 3.8 half-units, something tiny (for gcn_aggregate, whose
      weights there are 1 / 2).
A few generic rows hold the largest finite value, +-inf and NaN.

The conditions on the fp32 OUTPUTS are asserted per case (edge_shares): at least 1 % of the finite
outputs lie in S's subnormal range and - for an op that can exceed S's largest finite value - at
least 1 % round to inf.  Ops that cannot exceed it: max (a copy of an input), the unweighted means
and gcn's mean (|mean| <= the largest input), attention_aggregate (a convex combination),
edge_softmax (<= 1), gather_segment_topk and embedding_take (copies), and in bf16 the sqrtn
combiner (the sum that would be needed overflows fp32 first).

Shapes: 200 destinations, segment lengths 0 .. 20 (the 8 / 4 / 1 load batches all occur), about 2000
edges; per family one d on its widest store path and one on its element path."""
import numpy as np
import pytest

import half_edges as HE

pytestmark = pytest.mark.gpu

SIZE = 200
T1 = (3, 23, 43, 63, 83, 103)
T2 = (7, 27, 47, 67, 87, 107, 127, 147, 167, 187)
T4 = (11, 31, 52, 71, 91, 111)
N_TYPES = 3


def _S(torch, which):
    return [torch.bfloat16, torch.float16][which]


class Fmt:
    """constants of S as exact float64 numbers"""

    def __init__(self, torch, S):
        if S == torch.bfloat16:
            self.max, self.second, self.half = (2 - 2.0 ** -7) * 2.0 ** 127, (2 - 2.0 ** -6) * 2.0 ** 127, 2.0 ** 119
            self.ulp1 = 2.0 ** -7
            self.bands = ((-137, -124), (-3, 3), (123, 127))
        else:
            self.max, self.second, self.half, self.ulp1 = 65504.0, 65472.0, 16.0, 2.0 ** -10
            self.bands = ((-27, -13), (-3, 3), (12, 15))


class Block:
    """The edges of one sampled block and the values on them (numpy; built once per dtype, never
    modified).  Edges are stored grouped by destination; `perm` is a fixed shuffle of them."""

    def __init__(self, torch, S, seed=77):
        self.torch, self.S, self.f = torch, S, Fmt(torch, S)
        self.seed = seed
        rng = self.rng_for(0)
        lens = rng.integers(0, 21, SIZE)
        lens[::17] = 0                                  # empty destinations
        for group, n in ((T1, 1), (T2, 2), (T4, 4)):
            lens[list(group)] = n
        assert set(lens.tolist()) == set(range(21))     # every length occurs
        self.lens = lens
        self.seg = np.zeros(SIZE + 1, np.int64)
        self.seg[1:] = np.cumsum(lens)
        self.e = int(self.seg[-1])
        self.dst = np.repeat(np.arange(SIZE), lens).astype(np.int32)
        self.perm = rng.permutation(self.e)
        band = rng.integers(0, 3, SIZE)
        lo = np.array([self.f.bands[b][0] for b in band])
        hi = np.array([self.f.bands[b][1] for b in band])
        self.k_dst = rng.integers(lo, hi + 1)
        self.types = rng.integers(0, N_TYPES, self.e).astype(np.int32)
        self.types[rng.integers(0, self.e, 25)] = -1    # updates of no relation
        for r in T1 + T2 + T4:                          # a top destination is one bucket
            self.types[self.seg[r]:self.seg[r + 1]] = 1
        # generic rows that hold one special value throughout
        generic = np.flatnonzero(~np.isin(self.dst, T1 + T2 + T4))
        self.special = dict(zip(rng.choice(generic, 6, replace=False).tolist(),
                                [self.f.max, -self.f.max, np.inf, -np.inf, np.nan, np.inf]))
        self._x = {}

    def rng_for(self, *tag):
        """a generator of its own for every use, so that no value depends on the order of the tests"""
        return np.random.default_rng([self.seed, *tag])

    def t(self, a64, dtype=None):
        """float64 array -> a GPU tensor of S (or dtype); every value here is exact in fp32"""
        torch = self.torch
        return torch.from_numpy(np.array(a64, dtype=np.float64)).to(torch.float32).to(dtype or self.S).cuda()

    def banded(self, rng, k_rows, d, jitter=3):
        """[len(k_rows), d] values +- m * 2^(k - j), m in [1, 2), j in [0, jitter)"""
        n = len(k_rows)
        k = np.asarray(k_rows).reshape(n, 1) - rng.integers(0, jitter, (n, d))
        return np.ldexp(rng.choice([-1.0, 1.0], (n, d)) * (1 + rng.random((n, d))), k)

    def x(self, d):
        """[e, d] float64: the value of every edge and column (see the module's docstring)"""
        if d not in self._x:
            rng, f = self.rng_for(1, d), self.f
            v = self.banded(rng, self.k_dst[self.dst], d)
            for r in T1 + T2 + T4:
                b = int(self.seg[r])
                s = rng.choice([-1.0, 1.0], d)
                m = 1 + rng.integers(1, 8, d) / 8.0
                if r in T1:                             # (positive: a max keeps it)
                    v[b] = f.second
                elif r in T2:
                    v[b], v[b + 1] = s * f.max, s * f.half * m
                else:
                    v[b], v[b + 1], v[b + 2], v[b + 3] = s * f.max, s * f.max, s * 2 * f.half * m, s * f.half / 4096
            for p, val in self.special.items():
                v[p] = val
            v.setflags(write=False)
            self._x[d] = v
        return self._x[d]

    def weights(self, heads):
        """[e, heads] float64, exact in S: 2^-2 .. 2^2 times m; 1 + ulp on T1 edges, 1 on T2 / T4"""
        w = self.banded(self.rng_for(2, heads), np.zeros(self.e, np.int64) + 2, heads, jitter=5)
        for r in T1 + T2 + T4:
            w[self.seg[r]:self.seg[r + 1]] = 1 + self.f.ulp1 if r in T1 else 1.0
        return self.t(w).double().cpu().numpy()        # rounded to S once, here

    def dev(self, a, dtype):
        return self.torch.from_numpy(np.array(a)).to(dtype).cuda()


_BLOCKS = {}


@pytest.fixture
def blk(torch_cuda, which):
    S = _S(torch_cuda, which)
    if S not in _BLOCKS:
        _BLOCKS[S] = Block(torch_cuda, S)
    return _BLOCKS[S]


def edge_shares(out32, S):
    """(finite outputs, share of them in S's subnormal range, share that rounds to inf, classes)"""
    b = HE.bits32(out32)
    c = HE.classes(b[(b & 0x7fffffff) < 0x7f800000], S)
    n = max(c["n"], 1)
    return c["n"], c["subnormal"] / n, c["to_inf"] / n, c


def check_store(fn, S, what, overflow, torch, subnormal=True):
    """fn(out_dtype) -> the op's result; the contract, and the conditions on the fp32 outputs"""
    out32 = fn(torch.float32)
    outS = fn(S)
    assert out32.dtype == torch.float32 and outS.dtype == S and outS.shape == out32.shape, what
    n, sub, inf, c = edge_shares(out32, S)
    print("store-edges %-46s %-8s compared %6d  classes %s" % (what, str(S)[6:], out32.numel(), c))
    if subnormal:
        assert sub >= 0.01, (what, "subnormal share", sub, c)
    if overflow:
        assert inf >= 0.01, (what, "share that rounds to inf", inf, c)
    HE.assert_same16(outS, HE.round_cpu(out32, S), S, out32, what)


def forms(blk, d):
    """the per-edge rows as a table read through gather indices: params[gi] is x, edge by edge"""
    x = blk.x(d)
    shuffle = blk.rng_for(3, d).permutation(blk.e)
    gi = np.argsort(shuffle).astype(np.int32)
    return blk.t(x[shuffle]), blk.dev(gi, blk.torch.int32)


@pytest.mark.parametrize("d", [8, 20])
@pytest.mark.parametrize("which", [0, 1])
def test_scatter_reduces(EA, blk, which, d):
    torch, S, ops = blk.torch, blk.S, EA.ops
    x = blk.x(d)
    for order, sel in (("sorted", np.arange(blk.e)), ("shuffled", blk.perm)):
        xs, keys = blk.t(x[sel]), blk.dev(blk.dst[sel], torch.int32)
        for name, over in (("scatter_add", True), ("scatter_max", False), ("scatter_mean", False)):
            f = getattr(ops, name)
            check_store(lambda od: f(xs, keys, SIZE, out_dtype=od), S, "%s d=%d %s" % (name, d, order), over, torch)


@pytest.mark.parametrize("d", [8, 20])
@pytest.mark.parametrize("which", [0, 1])
def test_fused_reduces(EA, blk, which, d):
    """gather_scatter and gather_segment_reduce: unweighted, and with edge_weight in fp32 and in S.
    A weighted mean / max can exceed S's largest value through the product (the T1 destinations)."""
    torch, S, ops = blk.torch, blk.S, EA.ops
    params, gi = forms(blk, d)
    keys = blk.dev(blk.dst, torch.int32)
    seg_ptr = blk.dev(blk.seg, torch.int64)
    heads = 1 if d == 8 else 5                          # (d = 20, heads = 5: dh = 4, the element kernel)
    w64 = blk.weights(heads)
    for wname, w in (("", None), (" w=fp32", blk.t(w64, torch.float32)), (" w=S", blk.t(w64))):
        for mode in ("add", "max", "mean"):
            over = mode == "add" or w is not None
            check_store(lambda od: ops.gather_scatter(mode, params, gi, keys, SIZE, out_dtype=od, edge_weight=w),
                        S, "gather_scatter %s d=%d%s" % (mode, d, wname), over, torch)
            check_store(lambda od: ops.gather_segment_reduce(mode, params, gi, SIZE, seg_ptr=seg_ptr, out_dtype=od,
                                                             edge_weight=w),
                        S, "gather_segment_reduce %s d=%d%s" % (mode, d, wname), over, torch)


@pytest.mark.parametrize("d", [8, 3])
@pytest.mark.parametrize("which", [0, 1])
def test_segment_topk(EA, blk, which, d):
    """values are copies: the fill value (1e-7: an fp16 subnormal; -1e9: -inf in fp16) and the
    places of +-inf and NaN are the point"""
    torch, S, ops = blk.torch, blk.S, EA.ops
    params, gi = forms(blk, d)
    seg_ptr = blk.dev(blk.seg, torch.int64)
    for fill in (1e-7, -1e9):
        check_store(lambda od: ops.gather_segment_topk(params, gi, SIZE, 4, seg_ptr=seg_ptr, fill=fill,
                                                       out_dtype=od),
                    S, "gather_segment_topk d=%d fill=%g" % (d, fill), False, torch)


@pytest.mark.parametrize("d,heads", [(16, 2), (8, 2), (6, 2)])
@pytest.mark.parametrize("which", [0, 1])
def test_edge_dot(EA, blk, which, d, heads):
    """dh = 8, 4 and 3: the three chunk widths; every edge its own row of a, a random row of b
    (row 0 of b is ones, read by the `top` edges: largest + half-units in two columns of a head)"""
    torch, S, ops, f, rng = blk.torch, blk.S, EA.ops, blk.f, blk.rng_for(4, d)
    dh, e = d // heads, blk.e
    band = rng.integers(0, 3, e)
    k = rng.integers(np.array([f.bands[b][0] for b in band]), np.array([f.bands[b][1] for b in band]) + 1)
    a = blk.banded(rng, k, d)
    b = blk.banded(rng, np.zeros(300, np.int64) + 1, d)
    b[0] = 1.0
    bi = rng.integers(1, 300, e).astype(np.int32)
    top = rng.choice(e, e // 20, replace=False)
    for p in top:
        s = rng.choice([-1.0, 1.0], heads)
        row = np.full((heads, dh), f.half / 4096)
        row[:, 0], row[:, 1] = f.max, f.half * (1 + rng.integers(1, 8, heads) / 8.0)
        a[p] = (row * s.reshape(heads, 1)).reshape(-1)
    bi[top] = 0
    for p, val in zip(rng.choice(np.setdiff1d(np.arange(e), top), 4, replace=False), (np.inf, -np.inf, np.nan, f.max)):
        a[p] = val
    at, bt, bit = blk.t(a), blk.t(b), blk.dev(bi, torch.int32)
    check_store(lambda od: ops.edge_dot(at, None, bt, bit, heads=heads, out_dtype=od), S,
                "edge_dot d=%d heads=%d" % (d, heads), True, torch)


@pytest.mark.parametrize("d", [8, 20])
@pytest.mark.parametrize("which", [0, 1])
def test_gcn_aggregate(EA, blk, which, d):
    """every source row is read by one edge (norm_src = 1), so the weight of an edge is
    1 / sqrt(its destination's length): T4 lands beyond the largest value without a root, T1 with
    one (second-largest + 3.5 half-units)"""
    torch, S, ops, f = blk.torch, blk.S, EA.ops, blk.f
    x, src = forms(blk, d)
    keys = blk.dev(blk.dst, torch.int32)
    seg_ptr = blk.dev(blk.seg, torch.int64)
    root = blk.banded(blk.rng_for(5, d), blk.k_dst, d)
    for r in T1 + T2 + T4:
        root[r] = 3.5 * f.half if r in T1 else 0.0
    root = blk.t(root)
    size = (SIZE, blk.e)
    for op in ("add", "mean"):
        for rname, kw in (("", {}), (" root", {"root": root}), (" root alpha", {"root": root, "alpha": 0.25})):
            over = op == "add" and "alpha" not in kw
            check_store(lambda od: ops.gcn_aggregate(x, (keys, src), size, op=op, out_dtype=od, **kw), S,
                        "gcn_aggregate %s d=%d%s keys" % (op, d, rname), over, torch)
            check_store(lambda od: ops.gcn_aggregate(x, src, size, op=op, seg_ptr=seg_ptr, out_dtype=od, **kw), S,
                        "gcn_aggregate %s d=%d%s seg_ptr" % (op, d, rname), over, torch)


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("which", [0, 1])
def test_edge_softmax(EA, blk, which, heads):
    """no overflow class (outputs <= 1).  Half of a destination's logits are near 0 (its largest is
    0); the others reach down to where the output leaves S's normal range.  fp16: exp(x) is
    subnormal for x in -16.6 .. -9.7 (2^-24 .. 2^-14).  bf16: the library's exp returns +0 below
    -86 (mp_softmax.h: every exp is a normal fp32 number), so a subnormal output is
    exp(x) / s < 2^-126 with x >= -86: x < -87.3 + ln(s), which the sum s of a longer segment's
    near-zero half reaches (s > 3.8)."""
    torch, S, ops, rng = blk.torch, blk.S, EA.ops, blk.rng_for(6, heads)
    (lo, hi), near = ((-19.0, -8.0), -3.0) if S == torch.float16 else ((-86.2, -84.4), -0.5)
    logits = np.where(rng.random((blk.e, heads)) < 0.5, rng.uniform(lo, hi, (blk.e, heads)),
                      rng.uniform(near, 0.0, (blk.e, heads)))
    first = blk.seg[:-1][blk.lens > 0]
    logits[first] = 0.0
    x = blk.t(logits)
    keys = blk.dev(blk.dst[blk.perm], torch.int32)
    xs = blk.t(logits[blk.perm])
    seg_ptr = blk.dev(blk.seg, torch.int64)
    check_store(lambda od: ops.edge_softmax(x, seg_ptr=seg_ptr, out_dtype=od), S,
                "edge_softmax heads=%d seg_ptr" % heads, False, torch)
    check_store(lambda od: ops.edge_softmax(xs, indices=keys, size=SIZE, out_dtype=od), S,
                "edge_softmax heads=%d keys" % heads, False, torch)


@pytest.mark.parametrize("dv", [4, 3])
@pytest.mark.parametrize("which", [0, 1])
def test_attention_aggregate(EA, blk, which, dv):
    """dot (with v, and with v = None: q = 0, so alpha is uniform and k carries the values) and
    additive; dv = 4 stores packed pairs, dv = 3 single elements.  A convex combination: no
    overflow class."""
    torch, S, ops, rng = blk.torch, blk.S, EA.ops, blk.rng_for(7, dv)
    heads = 2
    d = heads * dv
    v, gi = forms(blk, d)
    rows = v.shape[0]
    seg_ptr = blk.dev(blk.seg, torch.int64)
    keys = blk.dev(blk.dst, torch.int32)
    q = blk.t(rng.standard_normal((SIZE, 8)))
    k = blk.t(rng.standard_normal((rows, 8)))
    check_store(lambda od: ops.attention_aggregate("dot", q, k, gi, SIZE, v=v, heads=heads, seg_ptr=seg_ptr,
                                                   out_dtype=od), S, "attention dot dv=%d seg_ptr" % dv, False, torch)
    check_store(lambda od: ops.attention_aggregate("dot", q, k, gi, SIZE, v=v, heads=heads, indices=keys,
                                                   out_dtype=od), S, "attention dot dv=%d keys" % dv, False, torch)
    q0 = torch.zeros((SIZE, d), dtype=S, device="cuda")
    check_store(lambda od: ops.attention_aggregate("dot", q0, v, gi, SIZE, heads=heads, seg_ptr=seg_ptr,
                                                   out_dtype=od), S, "attention dot dv=%d v=None" % dv, False, torch)
    qa = blk.t(rng.standard_normal((SIZE, heads)))
    ka = blk.t(rng.standard_normal((rows, heads)))
    check_store(lambda od: ops.attention_aggregate("additive", qa, ka, gi, SIZE, v=v, heads=heads, seg_ptr=seg_ptr,
                                                   out_dtype=od), S, "attention additive dv=%d" % dv, False, torch)


@pytest.mark.parametrize("d", [8, 20])
@pytest.mark.parametrize("which", [0, 1])
def test_relation_reduce(EA, blk, which, d):
    torch, S, ops = blk.torch, blk.S, EA.ops
    params, gi = forms(blk, d)
    et = blk.dev(blk.types, torch.int32)
    seg_ptr = blk.dev(blk.seg, torch.int64)
    keys = blk.dev(blk.dst, torch.int32)
    for op in ("add", "max", "mean", "mean_rel"):
        check_store(lambda od: ops.relation_reduce(op, params, gi, et, N_TYPES, SIZE, seg_ptr=seg_ptr, out_dtype=od),
                    S, "relation_reduce %s d=%d seg_ptr" % (op, d), op == "add", torch)
        check_store(lambda od: ops.relation_reduce(op, params, gi, et, N_TYPES, SIZE, indices=keys, out_dtype=od),
                    S, "relation_reduce %s d=%d keys" % (op, d), op == "add", torch)


@pytest.mark.parametrize("dim", [8, 5])
@pytest.mark.parametrize("which", [0, 1])
def test_sparse_feature_embedding(EA, O, blk, which, dim):
    """node r of the graph holds the entries [seg[r], seg[r + 1]) - the edges of destination r - and
    the table row of an entry is that edge's row"""
    torch, S = blk.torch, blk.S
    ids = np.arange(10, 10 + SIZE).astype(np.uint64)
    c = O.csr_from_raw(ids, np.arange(SIZE + 1, dtype=np.int64), np.roll(ids, -1), np.ones(SIZE, np.float32), 1)
    G = EA.Graph.from_csr(c.row_id, c.row_ptr, c.type_end, c.nbr, c.prefix_w, c.type_prefix, c.n_types,
                          sparse_features=(1, blk.seg, blk.lens.astype(np.int32), np.arange(blk.e).astype(np.uint64)))
    table = blk.t(blk.x(dim))
    nodes = torch.as_tensor(ids.astype(np.int64)).cuda()
    for combiner in ("sum", "mean", "sqrtn"):
        over = combiner == "sum" or (combiner == "sqrtn" and S == torch.float16)
        check_store(lambda od: G.sparse_feature_embedding(nodes, [0], [table], combiner, out_dtype=od)[0], S,
                    "sparse_feature_embedding %s dim=%d" % (combiner, dim), over, torch)


@pytest.mark.parametrize("d", [8, 20, 3])
@pytest.mark.parametrize("which", [0, 1])
def test_embedding_stores(EA, blk, which, d):
    """embedding_take(out_dtype), and the in-place stores with distinct ids: the same call on
    table.float(), rounded once on the CPU.  d = 8, 20 and 3: eight, four and one element a lane.
    update: fp32 values at every rounding edge (the ranged and tie patterns of half_edges, and
    values just past the largest finite one) into the 16-bit table; add: a table of largest values
    (and banded ones) plus half-units."""
    torch, S, ops, f, rng = blk.torch, blk.S, EA.ops, blk.f, blk.rng_for(8, d)
    x = blk.x(d)
    rows = blk.e
    table = blk.t(x)
    ids = blk.dev(rng.permutation(rows + 40)[:rows // 2] - 20, torch.int64)      # distinct; some name no row
    check_store(lambda od: ops.embedding_take(table, ids, out_dtype=od), S, "embedding_take d=%d" % d, False, torch)
    n = ids.numel()
    # update, fp32 values
    n_top = n * d // 40
    top32 = (rng.choice([-1.0, 1.0], n_top) * (f.max + f.half * (1 + rng.integers(1, 8, n_top) / 8.0)))
    assert np.isfinite(top32.astype(np.float32)).all()
    n_tie = n * d // 6
    bits = np.concatenate([top32.astype(np.float32).view(np.uint32), HE.tie_bits(S, n_tie, 32),
                           HE.ranged_bits(S, n * d - n_top - 3 * n_tie, 31)])
    values = HE.to_dev32(rng.permutation(bits)).view(n, d)
    t16, t32 = table.clone(), table.float()
    assert ops.embedding_update(t16, ids, values) is t16
    ops.embedding_update(t32, ids, values)
    _, sub, inf, c = edge_shares(t32, S)
    print("store-edges %-46s %-8s compared %6d  classes %s" % ("embedding_update d=%d" % d, str(S)[6:], t32.numel(), c))
    assert sub >= 0.01 and inf >= 0.01, c
    HE.assert_same16(t16, HE.round_cpu(t32, S), S, t32, "embedding_update d=%d" % d)
    # add: every 4th row of the table holds the largest value, the addend is 1.1 .. 1.9 half-units
    base = np.array(x)
    add = blk.banded(rng, blk.k_dst[blk.dst], d)
    top = np.arange(0, rows, 4)
    s = rng.choice([-1.0, 1.0], (top.size, d))
    base[top] = s * f.max
    add[top] = s * f.half * (1 + rng.integers(1, 8, (top.size, d)) / 8.0)
    for vname, vdt in (("fp32", torch.float32), ("S", S)):
        t16 = blk.t(base)
        t32 = t16.float()
        rid = torch.clamp(ids, 0, rows - 1)
        vals = blk.t(add, vdt)[rid]
        ops.embedding_add(t16, ids, vals)
        ops.embedding_add(t32, ids, vals.float())       # (widening is exact)
        what = "embedding_add d=%d values %s" % (d, vname)
        _, sub, inf, c = edge_shares(t32, S)
        print("store-edges %-46s %-8s compared %6d  classes %s" % (what, str(S)[6:], t32.numel(), c))
        assert sub >= 0.01 and inf >= 0.01, (what, c)
        HE.assert_same16(t16, HE.round_cpu(t32, S), S, t32, what)
