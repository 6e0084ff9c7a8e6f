"""The DEVICE forms of euler_amd/csrc/half_cvt.h - the casts the compiler lowers to the gfx950
convert instructions - against torch's CPU conversions, through the library's public entries.

tests/test_half_cvt_host.py pins the integer (host) forms to torch's CPU conversions on the
patterns of tests/half_edges.py; this file pins the device forms to the same reference on the same
patterns, so the two implementations of the header are tied to each other at every rounding
decision: fp16 subnormals produced and read, bf16 values that are fp32 subnormals, ties in both
directions, overflow to inf, infinities and NaNs.  Nothing on the right-hand side is computed on
the device.  The rule for a NaN is half_edges': it stays a NaN with the sign of the input - and,
as the header says, a quiet one."""
import numpy as np
import pytest

import half_edges as HE

pytestmark = pytest.mark.gpu

_P = {}


def _S(torch, which):
    return [torch.bfloat16, torch.float16][which]


def P(dtype):
    """the narrowing patterns of dtype (computed once) and their CPU rounding"""
    if dtype not in _P:
        p = HE.narrow_set(dtype)
        p.setflags(write=False)
        want = HE.round_cpu(p, dtype)
        want.setflags(write=False)
        _P[dtype] = (p, want)
    return _P[dtype]


def unaligned(torch, x):
    """the same values in a view that starts 2 bytes into its storage"""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    buf[1:] = x.reshape(-1)
    y = buf[1:].view(x.shape)
    assert y.data_ptr() % 16 == 2 and y.is_contiguous()
    return y


def table_graph(EA, O, val_bits, ends):
    """A graph of n nodes (ids 10 ..) whose dense feature rows are the rows of val_bits ([n, width]
    uint32 fp32 bits), cut into slots at `ends`: a uniform table.  -> (graph factory, ids)"""
    n, width = val_bits.shape
    assert ends[-1] == width
    ids = np.arange(10, 10 + n).astype(np.uint64)
    seg = np.arange(n + 1, dtype=np.int64)
    csr = O.csr_from_raw(ids, seg, ids.copy(), np.ones(n, np.float32), 1)
    feats = (len(ends), np.arange(n + 1, dtype=np.int64) * width, np.tile(np.array(ends, np.int32), n),
             np.ascontiguousarray(val_bits).view(np.float32).reshape(-1))

    def make():
        return EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w,
                                 csr.type_prefix, csr.n_types, csr.node_type, csr.node_weight,
                                 features=feats)
    return make, ids


# ---- widening -------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_gather_widens_every_pattern(EA, torch_cuda, which):
    """the scalar widen (d = 1; d = 8 from a 2-byte-aligned view) and the 8-wide widen (d = 8 in
    16-byte lanes) of all 65 536 patterns"""
    torch = torch_cuda
    S = _S(torch, which)
    b16 = HE.all16()
    want = HE.widen_cpu(b16, S)
    x = HE.to_dev16(b16, S)
    for what, view in (("element d=1", x.view(65536, 1)), ("lanes d=8", x.view(8192, 8)),
                       ("element d=8 unaligned", unaligned(torch, x.view(8192, 8)))):
        idx = torch.arange(view.shape[0], device="cuda", dtype=torch.int32)
        got = EA.ops.gather(view, idx, out_dtype=torch.float32)
        assert got.dtype == torch.float32 and got.shape == view.shape
        HE.assert_same32(got, want, b16 >> 15, what)
        assert HE.bits16(EA.ops.gather(view, idx)).tolist() == b16.tolist(), what     # a copy of the bits


@pytest.mark.parametrize("d", [8, 3])
@pytest.mark.parametrize("which", [0, 1])
def test_scatter_add_widens_every_pattern(EA, torch_cuda, which, d):
    """one update per destination: out = 0 + widen(x), fp32 - widen(x) with -0 -> +0"""
    torch = torch_cuda
    S = _S(torch, which)
    b16 = HE.all16()
    b16 = np.concatenate([b16, np.zeros((-b16.size) % d, np.uint16)])
    wide = HE.widen_cpu(b16, S)
    want = np.where(wide == 0x80000000, np.uint32(0), wide)
    x = HE.to_dev16(b16, S).view(-1, d)
    idx = torch.arange(x.shape[0], device="cuda", dtype=torch.int32)
    got = EA.ops.scatter_add(x, idx, x.shape[0], out_dtype=torch.float32)
    HE.assert_same32(got, want, b16 >> 15, "scatter_add d=%d" % d)


@pytest.mark.parametrize("which", [0, 1])
def test_feature_table_round_trip_on_the_device(EA, O, torch_cuda, which):
    """fp32 table of the widened non-NaN patterns -> set_dense_feature_dtype(S) (NarrowTableKernel)
    -> rows in S are the patterns, rows in fp32 their widening; dim 64 takes the 16-byte-lane
    kernel, dim 68 (four columns past the slot: zeros) the typed element kernel"""
    torch = torch_cuda
    S = _S(torch, which)
    b16 = HE.all16()
    b16 = b16[~HE.nan_mask16(b16, S)]
    b16 = np.concatenate([b16, np.zeros((-b16.size) % 64, np.uint16)]).reshape(-1, 64)
    wide = HE.widen_cpu(b16, S).reshape(b16.shape)
    make, ids = table_graph(EA, O, wide, [64])
    G = make()
    q = torch.as_tensor(ids.astype(np.int64)).cuda()
    got = G.get_dense_feature(q, [0], [64])[0]
    assert HE.bits32(got).tolist() == wide.reshape(-1).tolist(), "the fp32 table holds other bits"
    G.set_dense_feature_dtype(S)
    for dim in (64, 68):
        g16 = G.get_dense_feature(q, [0], [dim], out_dtype=S)[0]
        g32 = G.get_dense_feature(q, [0], [dim], out_dtype=torch.float32)[0]
        assert g16.dtype == S and g32.dtype == torch.float32
        assert not g16[:, 64:].view(torch.int16).any() and not g32[:, 64:].view(torch.int32).any()
        bad = np.flatnonzero(HE.bits16(g16[:, :64]) != b16.reshape(-1))
        assert bad.size == 0, (dim, [hex(int(b16.reshape(-1)[i])) for i in bad[:8]])
        HE.assert_same32(g32[:, :64], wide, b16.reshape(-1) >> 15, "dim %d" % dim)


# ---- narrowing ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_feature_table_narrows_like_the_cpu(EA, O, torch_cuda, which):
    """the scalar narrow on P: an fp32 table served in S (the typed element kernel's store), and
    the table converted by set_dense_feature_dtype(S) (NarrowTableKernel)"""
    torch = torch_cuda
    S = _S(torch, which)
    p, want = P(S)
    make, ids = table_graph(EA, O, p.reshape(-1, 64), [64])
    G = make()
    q = torch.as_tensor(ids.astype(np.int64)).cuda()
    got = G.get_dense_feature(q, [0], [64])[0]
    assert np.array_equal(HE.bits32(got), p), "the fp32 table holds other bits"
    HE.assert_same16(G.get_dense_feature(q, [0], [64], out_dtype=S)[0], want, S, p, "fp32 table, rows in S")
    G.set_dense_feature_dtype(S)
    HE.assert_same16(G.get_dense_feature(q, [0], [64], out_dtype=S)[0], want, S, p, "converted table")
    HE.assert_same16(G.get_dense_feature(q, [0], [68], out_dtype=S)[0][:, :64], want, S, p,
                  "converted table, element kernel")


@pytest.mark.parametrize("signs", [False, True])
@pytest.mark.parametrize("d,heads", [(64, 8), (3, 3)])
@pytest.mark.parametrize("which", [0, 1])
def test_weighted_reduce_store_narrows_like_the_cpu(EA, torch_cuda, which, d, heads, signs):
    """Narrow8 through Store8 (d = 64, heads = 8: 16-byte lanes, eight different weights a row) and
    StoreElem (d = 3, heads = 3) on P: one row of 1.0 in S, the fp32 weights hold P, one update
    per destination, so out = 0 + 1 * w: two correctly rounded fp32 operations that return w's
    bits except for -0 -> +0 and a NaN's payload.  signs: the row is +1, -1, +1, ... instead, so
    the two halves of a packed word differ in sign (a store that swapped them would show)."""
    torch = torch_cuda
    S = _S(torch, which)
    p, _ = P(S)
    p = np.concatenate([p, np.zeros((-p.size) % heads, np.uint32)])
    e, dh = p.size // heads, d // heads
    row = np.ones(d, np.float32)
    if signs:
        row[1::2] = -1
    w = p.view(np.float32).reshape(e, heads)
    with np.errstate(invalid="ignore"):
        want32 = (np.float32(0) + row.reshape(1, heads, dh) * w.reshape(e, heads, 1)).astype(np.float32)
    want32 = want32.reshape(-1).view(np.uint32)
    src = np.repeat(p.reshape(e, heads), dh, axis=1).reshape(-1)
    if not signs:       # the claim above, on the CPU
        keep = ~HE.nan_mask32(src) & (src != 0x80000000)
        assert np.array_equal(want32[keep], src[keep]) and np.all(want32[src == 0x80000000] == 0)
        assert np.array_equal(HE.nan_mask32(want32), HE.nan_mask32(src))
    ones = torch.from_numpy(row).cuda().to(S).view(1, d)
    gi = torch.zeros(e, device="cuda", dtype=torch.int32)
    si = torch.arange(e, device="cuda", dtype=torch.int32)
    wt = HE.to_dev32(p).view(e, heads)
    got32 = EA.ops.gather_scatter("add", ones, gi, si, e, edge_weight=wt, out_dtype=torch.float32)
    # (the sign of a NaN product is the hardware's own business: the store must keep it)
    HE.assert_same32(got32, want32, HE.bits32(got32) >> 31, "the fp32 result, not the store")
    gotS = EA.ops.gather_scatter("add", ones, gi, si, e, edge_weight=wt, out_dtype=S)
    assert gotS.dtype == S and gotS.shape == (e, d)
    HE.assert_same16(gotS, HE.round_cpu(want32, S), S, got32, "store d=%d" % d)
