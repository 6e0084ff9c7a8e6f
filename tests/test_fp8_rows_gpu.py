"""Quantised (fp8 e4m3fn + per-column scale) feature row tables on the device: conversions,
column absmax, gather and the gather_segment_reduce family, the table past 2^32 bytes and the
Python surface (ops.Fp8Rows, ops.column_absmax, Graph.fp8_dense_feature).

The contract has no tolerance: an op on a table has the bits of the fp32 op on its dequantised
values.  The reference is never the code under test: the dequantised table is formed on the CPU
(torch's float8_e4m3fn cast times the scale, one fp32 multiply) and fed to the numpy references
(mp_base_ref.py, weighted_mp_ref.py) and, uploaded as fp32, to the existing fp32 ops.  A 16-bit
out_dtype is one CPU rounding of the fp32 result."""
import os

import numpy as np
import pytest

import fp8_edges as E
import fp8_ref as R
import mp_base_ref as B
import weighted_mp_ref as WR
from conftest import ROOT

pytestmark = pytest.mark.gpu

OPS = ("add", "max", "mean")


def xhat_cpu(torch, q, scale):
    """the dequantised table by torch's CPU cast: float32(q) * scale, float32 numpy"""
    t = torch.from_numpy(np.ascontiguousarray(q, np.uint8)).view(torch.float8_e4m3fn).float()
    return (t * torch.from_numpy(np.asarray(scale, np.float32))).numpy()


def bits(a):
    """fp32 values (a tensor on any device, or an array) as uint32 bits"""
    if not isinstance(a, np.ndarray):
        assert str(a.dtype) == "torch.float32", a.dtype
        a = a.detach().cpu().numpy()
    assert a.dtype == np.float32, a.dtype
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what, nan_ok=False):
    """bit equality of fp32 results (a tensor or an array each); nan_ok: a NaN need only be a NaN"""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if nan_ok:
        gn, wn = (g & 0x7fffffff) > 0x7f800000, (w & 0x7fffffff) > 0x7f800000
        assert np.array_equal(gn, wn), (what, "NaN-ness differs")
        g, w = g[~wn], w[~wn]
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, (what, "%d of %d differ" % (bad.size, g.size),
                           [(int(i), hex(int(g.reshape(-1)[i])), hex(int(w.reshape(-1)[i]))) for i in bad[:6]])


def assert_same16(torch, got, want32, dtype, what):
    """a 16-bit result against ONE CPU rounding of the fp32 reference"""
    assert got.dtype == dtype, (what, got.dtype)
    want = torch.from_numpy(np.ascontiguousarray(want32, np.float32)).to(dtype)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), what


def make_table(rng, rows, d, nan_codes=False):
    """random codes (every finite code, -0 and the subnormals included) and scales with a full mantissa"""
    q = rng.integers(0, 256, (rows, d), dtype=np.int64).astype(np.uint8)
    if not nan_codes:
        q[(q & 0x7f) == 0x7f] = 0x35
    scale = (rng.uniform(0.5, 1.0, d) * np.exp2(rng.integers(-6, 7, d))).astype(np.float32)
    return q, scale


def upload(torch, EA, q, scale):
    return EA.ops.Fp8Rows(torch.from_numpy(q).cuda(), torch.from_numpy(scale).cuda())


# ---- conversions on the device ---------------------------------------------------------------
@pytest.mark.parametrize("layout", ["d1", "d16", "d16_offset", "d16_odd"])
def test_every_code_decodes_as_on_the_cpu(EA, torch_cuda, layout):
    torch = torch_cuda
    rng = np.random.default_rng(50)
    d = 1 if layout == "d1" else 16
    q = ((np.arange(256)[:, None] + 16 * np.arange(d)[None, :]) % 256).astype(np.uint8)
    assert all(sorted(q[:, c].tolist()) == list(range(256)) for c in range(d))
    if layout in ("d16_offset", "d16_odd"):
        # a view offset by one row of a d = 20 table is 4-byte aligned only: fp32 rows by the four-code
        # lanes, 16-bit rows by the element path; one byte more and fp32 rows take the element path too
        off = 20 if layout == "d16_offset" else 21
        buf = torch.zeros(off + 256 * 16, dtype=torch.uint8, device="cuda")
        qd = buf[off:].view(256, 16)
        qd.copy_(torch.from_numpy(q))
        assert qd.data_ptr() % 16 == off % 16 and qd.data_ptr() % 4 == off % 4 and qd.is_contiguous()
    else:
        qd = torch.from_numpy(q).cuda()
        assert qd.data_ptr() % 16 == 0
    idx = torch.arange(256, device="cuda", dtype=torch.int32)
    for scale in (np.ones(d, np.float32), (rng.uniform(0.5, 1.0, d) * 3).astype(np.float32)):
        T = EA.ops.Fp8Rows(qd, torch.from_numpy(scale).cuda())
        assert T.q.data_ptr() == qd.data_ptr() and tuple(T.shape) == (256, d) and T.device == qd.device
        want = xhat_cpu(torch, q, scale)
        assert np.isnan(want).sum() == 2 * d
        for got in (EA.ops.gather(T, idx), T.dequantize(), EA.ops.gather(T, idx, out_dtype=torch.float32)):
            assert got.dtype == torch.float32 and not got.requires_grad
            assert_same(got, want, layout, nan_ok=True)
        keep = ~np.isnan(want)
        for dt in (torch.bfloat16, torch.float16):
            got = EA.ops.gather(T, idx, out_dtype=dt)
            w16 = torch.from_numpy(want).to(dt)
            k = torch.from_numpy(keep)
            assert got.dtype == dt and torch.equal(got.cpu().view(torch.int16)[k], w16.view(torch.int16)[k])
            assert torch.isnan(got.cpu().float()[~k]).all()


@pytest.mark.parametrize("cols", [16, 3])
@pytest.mark.parametrize("src", ["float32", "bfloat16", "float16"])
def test_quantize_equals_the_reference_on_the_edge_set(EA, torch_cuda, cols, src):
    torch = torch_cuda
    dt = getattr(torch, src)
    p = np.array(E.encode_set())
    x = torch.from_numpy(p.view(np.int32)).view(torch.float32).reshape(-1, cols).to(dt)      # (CPU rounding)
    x32 = x.float().numpy()                          # what the kernel sees after its exact widening
    rng = np.random.default_rng(51)
    inexact = (rng.uniform(0.5, 1.0, cols) * np.exp2(rng.integers(-2, 3, cols)) * 1.37).astype(np.float32)
    xd = x.cuda()
    for scale in (np.ones(cols, np.float32), inexact):
        T = EA.ops.Fp8Rows.quantize(xd, torch.from_numpy(scale).cuda())
        got = T.q.cpu().numpy()
        want = R.quantize(x32, scale)
        nan_in = np.isnan(x32)
        assert np.array_equal(got[~nan_in], want[~nan_in]), \
            [(hex(int(a)), hex(int(b))) for a, b in zip(got[~nan_in][got[~nan_in] != want[~nan_in]][:6],
                                                        want[~nan_in][got[~nan_in] != want[~nan_in]][:6])]
        sign = (x32.view(np.uint32) >> 24).astype(np.uint8) & 0x80
        assert np.array_equal(got[nan_in], (sign | 0x7f)[nan_in])
        assert torch.equal(T.q.view(torch.float8_e4m3fn).view(torch.uint8), T.q)
        assert T.q.view(torch.float8_e4m3fn).data_ptr() == T.q.data_ptr()
    if src == "float32" and cols == 16:              # scale 1: the reference is torch's own clamped cast
        T = EA.ops.Fp8Rows.quantize(xd, torch.ones(cols, device="cuda"))
        assert E.enc_mismatches(T.q.cpu().numpy(), p).size == 0


@pytest.mark.parametrize("src", ["float32", "bfloat16", "float16"])
def test_column_absmax_whole_and_in_chunks(EA, torch_cuda, src):
    torch = torch_cuda
    dt = getattr(torch, src)
    rng = np.random.default_rng(52)
    x = (rng.standard_normal((1000, 70)) * np.exp2(rng.integers(-10, 10, (1000, 70)))).astype(np.float32)
    x[:, 2] = 0
    x[:, 5] = np.where(rng.random(1000) < 0.5, np.nan, np.inf)
    x[3, 6], x[4, 6], x[5, 6] = np.nan, np.inf, -np.inf
    x[:, 69] = -np.abs(x[:, 69])
    xt = torch.from_numpy(x).to(dt)
    want = R.column_absmax(xt.float().numpy())
    assert want[2] == 0 and want[5] == 0 and want[6] > 0
    xd = xt.cuda()
    got = EA.ops.column_absmax(xd)
    assert got.dtype == torch.float32 and tuple(got.shape) == (70,)
    assert_same(got, want, "whole")
    out = torch.zeros(70, device="cuda")
    for lo, hi in ((0, 1), (1, 400), (400, 1000)):
        assert EA.ops.column_absmax(xd[lo:hi], out=out) is out
    assert_same(out, want, "chunks")
    assert_same(EA.ops.Fp8Rows.scale_of(got), R.scale_of(want), "scale")
    assert_same(EA.ops.column_absmax(xd[:, :1].contiguous()), want[:1], "d = 1")
    T = EA.ops.Fp8Rows.quantize(xd)
    assert_same(T.scale, R.scale_of(want), "quantize's scale")
    x32 = xt.float().numpy()
    assert np.array_equal(T.q.cpu().numpy()[~np.isnan(x32)], R.quantize(x32, R.scale_of(want))[~np.isnan(x32)])


# ---- reduces -----------------------------------------------------------------------------------
def _check_reduce(torch, EA, T, xh, xh_dev, op, gi, size, seg_ptr=None, count=None, ids=False, out16=None):
    """the three comparisons of one call; gi: numpy indices (ids: int64 ids read in place)"""
    rows = xh.shape[0]
    gi_dev = torch.from_numpy(np.asarray(gi, np.int64 if ids else np.int32)).cuda()
    sp_dev = None if seg_ptr is None else torch.from_numpy(np.asarray(seg_ptr, np.int64)).cuda()
    kw = dict(seg_ptr=sp_dev, count=count)
    got = EA.ops.gather_segment_reduce(op, T, gi_dev, size, **kw)
    assert got.dtype == torch.float32 and not got.requires_grad and tuple(got.shape) == (size, xh.shape[1])
    keys = B.segment_keys(size, seg_ptr, count)
    r = B.id_rows(gi, rows) if ids else np.asarray(gi)
    what = (op, xh.shape, size, count, "ids" if ids else "i32")
    want = B.gather_scatter_ref(op, xh, r, keys, size)
    assert_same(got, want, what + ("numpy",))
    assert_same(got, EA.ops.gather_segment_reduce(op, xh_dev, gi_dev, size, **kw), what + ("fp32 op",))
    assert_same(EA.ops.gather_segment_reduce(op, T, gi_dev, size, out_dtype=torch.float32, **kw), want, what)
    if out16 is not None:
        assert_same16(torch, EA.ops.gather_segment_reduce(op, T, gi_dev, size, out_dtype=out16, **kw), want,
                      out16, what + (out16,))


COUNTS = (1, 3, 4, 5, 8, 9, 17, 25)
SIZES = (1, 5, 257)


@pytest.mark.parametrize("d", [1, 8, 16, 20, 48, 128, 144, 512, 1040])
def test_count_reduces_meet_the_contract(EA, torch_cuda, d):
    """every op x every count (the unroll edges 8 / 4 / 1 of the row pipeline), the sizes and table
    rows rotating so that each meets every op; int32 indices and int64 ids"""
    torch = torch_cuda
    rng = np.random.default_rng(60 + d)
    tables = []
    for rows in (1, 300):
        q, scale = make_table(rng, rows, d)
        xh = xhat_cpu(torch, q, scale)
        assert_same(xh, R.dequantize(q, scale), "the two CPU dequantisations")
        tables.append((upload(torch, EA, q, scale), xh, torch.from_numpy(xh).cuda()))
    k = 0
    for ci, count in enumerate(COUNTS):
        for oi, op in enumerate(OPS):
            size = SIZES[(ci + oi) % 3]
            T, xh, xh_dev = tables[(ci + oi + 1) % 2 if size != 257 else 1]
            rows = xh.shape[0]
            ids = k % 2 == 1
            gi = rng.integers(0, rows, size * count)
            if ids:                                   # -1 and ids past the table read the last row
                gi = gi.astype(np.int64)
                gi[::5] = -1
                gi[1::7] = rows + rng.integers(0, 1 << 40, gi[1::7].size)
            out16 = (torch.bfloat16, torch.float16, None)[k % 3]
            _check_reduce(torch, EA, T, xh, xh_dev, op, gi, size, count=count, ids=ids, out16=out16)
            k += 1
    # every size with every op at one count, on the one-row table too
    for op in OPS:
        for size in SIZES:
            for T, xh, xh_dev in tables:
                gi = rng.integers(0, xh.shape[0], size * 9)
                _check_reduce(torch, EA, T, xh, xh_dev, op, gi, size, count=9)


@pytest.mark.parametrize("d", [1, 16, 20, 48, 128, 1040])
def test_seg_ptr_reduces_meet_the_contract(EA, torch_cuda, d):
    torch = torch_cuda
    rng = np.random.default_rng(70 + d)
    q, scale = make_table(rng, 300, d)
    xh = xhat_cpu(torch, q, scale)
    T, xh_dev = upload(torch, EA, q, scale), torch.from_numpy(xh).cuda()
    lens = [0, 1, 7, 0, 8, 9, 33, 0]                  # empty first, middle and last segments
    seg_ptr = np.concatenate([[0], np.cumsum(lens)])
    for k, op in enumerate(OPS):
        gi = rng.integers(0, 300, int(seg_ptr[-1]))
        _check_reduce(torch, EA, T, xh, xh_dev, op, gi, len(lens), seg_ptr=seg_ptr,
                      out16=(torch.bfloat16, torch.float16)[k % 2])
        ids = gi.astype(np.int64)
        ids[::4] = -1
        ids[1::6] = 300 + (1 << 33)
        _check_reduce(torch, EA, T, xh, xh_dev, op, ids, len(lens), seg_ptr=seg_ptr, ids=True)
    got = EA.ops.gather_segment_reduce("max", T, torch.from_numpy(gi).cuda(), len(lens),
                                       seg_ptr=torch.from_numpy(seg_ptr).cuda())
    assert (got[[0, 3, 7]] == -1e9).all()             # the empty max row
    # validate=True looks at the indices first
    bad = torch.tensor([0, 1, 300], dtype=torch.int64, device="cuda")
    with pytest.raises(IndexError):
        EA.ops.gather_segment_reduce("add", T, bad, 1, count=3, validate=True)
    with pytest.raises(IndexError):
        EA.ops.gather_segment_reduce("add", T, torch.tensor([0, -1, 2], device="cuda"), 1, count=3, validate=True)
    ok = torch.tensor([0, 299, 2], dtype=torch.int64, device="cuda")
    assert_same(EA.ops.gather_segment_reduce("add", T, ok, 1, count=3, validate=True),
                B.gather_scatter_ref("add", xh, [0, 299, 2], [0, 0, 0], 1), "validated")


@pytest.mark.parametrize("d", [16, 20, 48, 128])
def test_weighted_reduces_meet_the_contract(EA, torch_cuda, d):
    torch = torch_cuda
    rng = np.random.default_rng(80 + d)
    q, scale = make_table(rng, 300, d)
    xh = xhat_cpu(torch, q, scale)
    T, xh_dev = upload(torch, EA, q, scale), torch.from_numpy(xh).cuda()
    k = 0
    for heads in (1, 4, d):
        for wdt in (torch.float32, torch.bfloat16):
            for op in OPS:
                size, count = (5, 9) if k % 2 else (257, 5)
                seg_ptr = None
                if k % 3 == 2:
                    lens = rng.integers(0, 12, size)
                    lens[0] = lens[-1] = 0
                    seg_ptr, count = np.concatenate([[0], np.cumsum(lens)]), None
                e = size * count if seg_ptr is None else int(seg_ptr[-1])
                ids = k % 4 == 1
                gi = rng.integers(0, 300, e)
                if ids:
                    gi = gi.astype(np.int64)
                    gi[::5] = -1
                w = torch.from_numpy(rng.standard_normal((e, heads)).astype(np.float32)).to(wdt)
                w32 = w.float().numpy()                                  # (widening is exact)
                gi_dev = torch.from_numpy(np.asarray(gi, np.int64 if ids else np.int32)).cuda()
                sp_dev = None if seg_ptr is None else torch.from_numpy(seg_ptr).cuda()
                kw = dict(seg_ptr=sp_dev, count=count)
                got = EA.ops.gather_segment_reduce(op, T, gi_dev, size, edge_weight=w.cuda(), **kw)
                assert got.dtype == torch.float32 and not got.requires_grad
                r = B.id_rows(gi, 300) if ids else gi
                want = WR.gather_scatter_ref(op, xh, r, WR.segment_dst(size, seg_ptr, count), size, w32)
                what = (op, d, heads, wdt, size, count, ids)
                assert_same(got, want, what + ("numpy",))
                assert_same(got, EA.ops.gather_segment_reduce(op, xh_dev, gi_dev, size,
                                                              edge_weight=w.float().cuda(), **kw), what + ("fp32 op",))
                dt16 = (torch.bfloat16, torch.float16)[k % 2]
                assert_same16(torch, EA.ops.gather_segment_reduce(op, T, gi_dev, size, edge_weight=w.cuda(),
                                                                  out_dtype=dt16, **kw), want, dt16, what)
                k += 1
    w = torch.ones(15, 1, device="cuda", requires_grad=True)
    gi_dev = torch.zeros(15, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError):
        EA.ops.gather_segment_reduce("add", T, gi_dev, 5, count=3, edge_weight=w)
    with pytest.raises(ValueError):
        EA.ops.gather_segment_reduce("add", T, gi_dev, 5, count=3, edge_weight=torch.ones(15, 7, device="cuda"))
    with pytest.raises(TypeError):
        EA.ops.gather_segment_reduce("add", T, gi_dev, 5, count=3,
                                     edge_weight=torch.ones(15, 1, device="cuda", dtype=torch.float64))


@pytest.mark.parametrize("d", [16, 20])
def test_a_table_with_nan_codes(EA, torch_cuda, d):
    """NaN-ness and every non-NaN output agree (a NaN's payload is nobody's contract)"""
    torch = torch_cuda
    rng = np.random.default_rng(90 + d)
    q, scale = make_table(rng, 300, d, nan_codes=True)
    q[::3] = np.where((q[::3] & 0x7f) == 0x7f, 0x11, q[::3])      # (rows without one too)
    assert ((q & 0x7f) == 0x7f).sum() > 10
    xh = xhat_cpu(torch, q, scale)
    T, xh_dev = upload(torch, EA, q, scale), torch.from_numpy(xh).cuda()
    assert_same(T.dequantize(), xh, "dequantize", nan_ok=True)
    for op in OPS:
        gi = rng.integers(0, 300, 257 * 5)
        gi_dev = torch.from_numpy(gi.astype(np.int32)).cuda()
        got = EA.ops.gather_segment_reduce(op, T, gi_dev, 257, count=5)
        with np.errstate(invalid="ignore"):
            want = B.gather_scatter_ref(op, xh, gi, B.segment_keys(257, None, 5), 257)
        assert_same(got, want, (op, "numpy"), nan_ok=True)
        assert_same(got, EA.ops.gather_segment_reduce(op, xh_dev, gi_dev, 257, count=5), (op, "fp32 op"), nan_ok=True)
        assert np.isnan(want).any() == (op != "max") and not np.isnan(want).all()


# ---- past 2^32 bytes -----------------------------------------------------------------------------
def test_a_table_past_4_gib(EA, torch_cuda):
    torch = torch_cuda
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory, %.1f GiB are free" % (free / 2.0 ** 30))
    n, d = (1 << 25) + 8, 128
    assert n * d == (1 << 32) + 1024
    rng = np.random.default_rng(95)
    # the rows around byte offsets 2^31 and 2^32, and the last row
    hot = np.array([(1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 25) - 1, 1 << 25, (1 << 25) + 1, n - 1], np.int64)
    small_q, scale = make_table(rng, hot.size, d)
    small_q[(small_q & 0x7f) == 0] = 0x41              # (no zero of either sign among the hot values)
    big = torch.zeros((n, d), dtype=torch.uint8, device="cuda")
    big[torch.from_numpy(hot).cuda()] = torch.from_numpy(small_q).cuda()
    T = EA.ops.Fp8Rows(big, torch.from_numpy(scale).cuda())
    xh = xhat_cpu(torch, small_q, scale)
    assert np.count_nonzero(xh) == xh.size
    # gather: the hot rows, and their neighbours outside the set (zero rows)
    idx = np.concatenate([hot, hot[:6] + 3, [0]])
    got = EA.ops.gather(T, torch.from_numpy(idx.astype(np.int32)).cuda())
    assert_same(got[:hot.size], xh, "gather past 2^32 bytes")
    assert int(torch.count_nonzero(got)) == xh.size
    # count-3 mean over exactly those rows, by int32 indices and by int64 ids
    pick = rng.integers(0, hot.size, 3 * 64)
    want = B.gather_scatter_ref("mean", xh, pick, B.segment_keys(64, None, 3), 64)
    for dt in (np.int32, np.int64):
        gi = torch.from_numpy(hot[pick].astype(dt)).cuda()
        got = EA.ops.gather_segment_reduce("mean", T, gi, 64, count=3)
        assert_same(got, want, ("mean past 2^32 bytes", dt))
        assert int(torch.count_nonzero(got)) == np.count_nonzero(want) and np.count_nonzero(want) > 64 * 100
    ids = hot[pick].copy()
    ids[::4] = n + (1 << 35)                           # past the table: its last row
    pick2 = pick.copy()
    pick2[::4] = hot.size - 1
    got = EA.ops.gather_segment_reduce("mean", T, torch.from_numpy(ids).cuda(), 64, count=3)
    assert_same(got, B.gather_scatter_ref("mean", xh, pick2, B.segment_keys(64, None, 3), 64), "ids past the table")
    del big, T


# ---- the Python surface --------------------------------------------------------------------------
def test_store_in_chunks_and_the_surface(EA, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(96)
    x = torch.from_numpy((rng.standard_normal((1000, 24)) * 5).astype(np.float32)).cuda()
    whole = EA.ops.Fp8Rows.quantize(x)
    assert whole.q.dtype == torch.uint8 and whole.scale.dtype == torch.float32
    assert tuple(whole.shape) == (1000, 24) and whole.device == x.device
    T = EA.ops.Fp8Rows.empty(1000, 24, whole.scale, x.device)
    T.q.fill_(0x55)
    for lo, hi in ((0, 1), (400, 1000), (1, 400)):
        assert T.store(lo, x[lo:hi]) is T
    assert torch.equal(T.q, whole.q)
    with pytest.raises(IndexError):
        T.store(999, x[:2])
    with pytest.raises(ValueError):
        T.store(0, x[:, :8])
    # a caller's scale that clips: values past it saturate
    clip = EA.ops.Fp8Rows.quantize(x, whole.scale / 4)
    assert np.array_equal(clip.q.cpu().numpy(), R.quantize(x.cpu().numpy(), (whole.scale / 4).cpu().numpy()))
    assert ((clip.q & 0x7f) == 0x7e).sum() > 24
    # the same bytes as a float8 tensor
    f8 = whole.q.view(torch.float8_e4m3fn)
    assert f8.data_ptr() == whole.q.data_ptr()
    assert torch.equal(EA.ops.Fp8Rows(f8, whole.scale).q, whole.q)
    assert_same(whole.dequantize(), (f8.cpu().float() * whole.scale.cpu()).numpy(), "dequantize vs torch")
    assert whole.dequantize(torch.bfloat16).dtype == torch.bfloat16
    # no gradient flows: not from the source tensor, not into any output
    xr = x.clone().requires_grad_(True)
    Tr = EA.ops.Fp8Rows.quantize(xr)
    assert not Tr.q.requires_grad and not Tr.scale.requires_grad and torch.equal(Tr.q, whole.q)
    idx = torch.arange(10, device="cuda")
    assert not EA.ops.gather(Tr, idx).requires_grad
    assert not EA.ops.gather_segment_reduce("mean", Tr, idx, 5, count=2).requires_grad
    # tensors of other dtypes raise exactly what they raise today
    for bad in (f8, whole.q, x.double(), x.to(torch.int32)):
        with pytest.raises(TypeError, match="data must be float32, bfloat16 or float16"):
            EA.ops.gather(bad, idx)
        with pytest.raises(TypeError, match="data must be float32, bfloat16 or float16"):
            EA.ops.gather_segment_reduce("add", bad, idx, 5, count=2)
    with pytest.raises(TypeError):
        EA.ops.gather(whole, idx, out_dtype=torch.float64)
    with pytest.raises(TypeError):
        EA.ops.gather_segment_reduce("add", whole, idx, 5, count=2, out_dtype=torch.int8)
    with pytest.raises(ValueError):
        EA.ops.gather_segment_reduce("min", whole, idx, 5, count=2)
    with pytest.raises(ValueError):
        EA.ops.gather_segment_reduce("add", whole, idx, 5)
    with pytest.raises(TypeError):
        EA.ops.Fp8Rows(whole.q, whole.scale.double())
    with pytest.raises(RuntimeError):
        EA.ops.Fp8Rows(whole.q.cpu(), whole.scale.cpu())
    # empty shapes
    assert tuple(EA.ops.gather(whole, idx[:0]).shape) == (0, 24)
    assert tuple(EA.ops.gather_segment_reduce("add", whole, idx[:0], 0, count=3).shape) == (0, 24)


def _check_graph_table(torch, EA, G, fid, dim, chunk_rows):
    max_id = int(G.id_range()[0])
    ids = torch.arange(max_id + 1, dtype=torch.int64, device="cuda")
    x = G.get_dense_feature(ids, [fid], [dim])[0]
    want = EA.ops.Fp8Rows.quantize(x)
    got = G.fp8_dense_feature(fid, dim, chunk_rows=chunk_rows)
    assert tuple(got.shape) == (max_id + 1, dim)
    assert torch.equal(got.scale, want.scale) and torch.equal(got.q, want.q)
    assert np.array_equal(got.q.cpu().numpy(), R.quantize(x.cpu().numpy(), R.column_scale(x.cpu().numpy())))
    return got, x


def test_graph_fp8_dense_feature(EA, O, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(97)
    n = 3000
    ids = np.arange(10, 10 + n).astype(np.uint64)
    csr = O.csr_from_raw(ids, np.arange(n + 1, dtype=np.int64) * 3, rng.choice(ids, 3 * n),
                         np.ones(3 * n, np.float32), 1)
    val = (rng.standard_normal((n, 40)) * np.exp2(rng.integers(-3, 4, 40))).astype(np.float32)
    feats = (2, np.arange(n + 1, dtype=np.int64) * 40, np.tile(np.array([32, 40], np.int32), n), val.reshape(-1))
    G = EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w, csr.type_prefix,
                          csr.n_types, csr.node_type, csr.node_weight, features=feats)
    before = G.device_bytes
    T, x = _check_graph_table(torch, EA, G, 0, 32, chunk_rows=1000)      # (3010 ids: a ragged last chunk)
    assert not T.q[:10].any() and T.q[10:].any()                         # ids 0 .. 9 are no nodes: zero rows
    assert G.device_bytes == before and G.dense_feature_dtype == torch.float32      # no new graph state
    _check_graph_table(torch, EA, G, 1, 8, chunk_rows=1 << 20)
    # the block mean over sampled ids, read in place: the bits of the fp32 op on dequantize()
    G.set_seed(3)
    roots = torch.from_numpy(rng.choice(ids, 64).astype(np.int64)).cuda()
    nb = G.sample_fanout(roots, [[0]], [5], -1, call_id=1)[0][1]
    got = EA.ops.gather_segment_reduce("mean", T, nb, 64, count=5)
    assert_same(got, EA.ops.gather_segment_reduce("mean", T.dequantize(), nb, 64, count=5), "block mean")
    # the ragged fixture table: unknown ids and short slots give zero rows / columns
    F = EA.Graph.load(os.path.join(ROOT, "tests", "golden", "fixture_dat"))
    fg = np.load(os.path.join(ROOT, "tests", "golden", "features.npz"))
    for fid in range(int(fg["fx_n_float"])):
        for dim, chunk in ((1, 7), (40, 1 << 20)):
            _check_graph_table(torch, EA, F, fid, dim, chunk)
    T, x = _check_graph_table(torch, EA, F, int(fg["fx_n_float"]) + 2, 5, 16)      # a slot that does not exist
    assert not T.q.any() and bool((T.scale == 1).all())
