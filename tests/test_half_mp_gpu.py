"""bf16 / fp16 storage for the message-passing ops and the dense feature table.

Contract (include/euler_gpu.h, DESIGN): for an op f, storage dtype S and input x of dtype S,
f_S(x, out_dtype=fp32) has the bits of f_fp32(x.float()) and f_S(x, out_dtype=S) the bits of
f_fp32(x.float()).to(S).  Every comparison here is torch.equal on the integer view of the
result; the right-hand side is computed with the existing fp32 ops and torch's own
conversions.  Inputs are finite with |x| <= 4 so that sums stay finite in fp16."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

DIMS = [1, 3, 8, 20, 64, 128, 200, 256, 512, 520]
MODES = ["add", "max", "mean"]


def _S(torch):
    return [torch.bfloat16, torch.float16]


def bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same(got, want):
    import torch
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(bits(got), bits(want))


def draw(torch, gen, shape, S, unaligned=False):
    """values of dtype S in [-4, 4]; unaligned: a view that starts 2 bytes into its storage
    (2-byte but not 16-byte aligned)"""
    x = ((torch.rand(shape, generator=gen, device="cuda") * 8) - 4).to(S)
    if unaligned:
        buf = torch.empty(x.numel() + 1, dtype=S, device="cuda")
        buf[1:] = x.reshape(-1)
        x = buf[1:].view(shape)
        assert x.data_ptr() % 16 == 2 and x.is_contiguous()
    return x


def check_op(torch, fn, x, S):
    """fn(data, out_dtype) -> result, for data = x (dtype S) and data = x.float()"""
    want32 = fn(x.float(), None)
    assert want32.dtype == torch.float32
    got32 = fn(x, torch.float32)
    assert same(got32, want32), "out fp32"
    gotS = fn(x, S)
    assert same(gotS, want32.to(S)), "out S"
    assert same(fn(x, None), gotS), "out_dtype=None is the input's dtype"


@pytest.fixture(scope="module")
def gen(torch_cuda):
    g = torch_cuda.Generator(device="cuda")
    g.manual_seed(1234)
    return g


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("which", [0, 1])
def test_scatter_ops_meet_the_contract(EA, torch_cuda, gen, which, d):
    """scatter_add / max / mean: sorted and shuffled keys, empty destinations, keys >= size,
    aligned and 2-byte-aligned input"""
    torch = torch_cuda
    S = _S(torch)[which]
    ops = EA.ops
    e, size = 1500, 120
    keys = torch.randint(0, size + 15, (e,), generator=gen, device="cuda", dtype=torch.int32)
    keys[(keys % 7) == 3] += 1                         # destinations 3, 10, 17, ... stay empty
    for order in ("sorted", "shuffled"):
        idx = torch.sort(keys).values if order == "sorted" else keys
        for unaligned in (False, True):
            x = draw(torch, gen, (e, d), S, unaligned)
            for mode in MODES:
                check_op(torch, lambda t, od: ops.scatter_(mode, t, idx, size, out_dtype=od), x, S)
    # the named entry points
    x = draw(torch, gen, (e, d), S)
    for name in ("scatter_add", "scatter_max", "scatter_mean"):
        f = getattr(ops, name)
        check_op(torch, lambda t, od: f(t, keys, size, out_dtype=od), x, S)
    out = ops.scatter_max(x, keys, size)
    empty = torch.full((d,), -1e9, device="cuda").to(S)
    assert same(out[3], empty)                         # -1e9 rounded to S (-inf in fp16)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("which", [0, 1])
def test_gather_and_fused_reduces_meet_the_contract(EA, torch_cuda, gen, which, d):
    torch = torch_cuda
    S = _S(torch)[which]
    ops = EA.ops
    rows, size, count = 300, 90, 10
    for unaligned in (False, True):
        x = draw(torch, gen, (rows, d), S, unaligned)
        gi = torch.randint(0, rows, (size * count,), generator=gen, device="cuda", dtype=torch.int32)
        check_op(torch, lambda t, od: ops.gather(t, gi, out_dtype=od), x, S)
        assert same(ops.gather(x, gi), x[gi.long()])          # equal dtypes: the stored bits
        si = torch.randint(0, size + 5, (size * count,), generator=gen, device="cuda", dtype=torch.int32)
        lens = torch.randint(0, 23, (size,), generator=gen, device="cuda")
        lens[::9] = 0
        seg_ptr = torch.zeros(size + 1, dtype=torch.int64, device="cuda")
        seg_ptr[1:] = torch.cumsum(lens, 0)
        gp = torch.randint(0, rows, (int(seg_ptr[-1]),), generator=gen, device="cuda", dtype=torch.int32)
        ids = torch.randint(0, rows + 40, (size * count,), generator=gen, device="cuda", dtype=torch.int64)
        ids[::13] = -1                                 # default_node: reads the last row
        ids[5::17] += 1 << 33                          # only the low word counts
        for mode in MODES:
            for s_idx in (si, torch.sort(si).values):
                check_op(torch, lambda t, od: ops.gather_scatter(mode, t, gi, s_idx, size, out_dtype=od), x, S)
            check_op(torch, lambda t, od: ops.gather_segment_reduce(mode, t, gi, size, count=count,
                                                                    out_dtype=od), x, S)
            check_op(torch, lambda t, od: ops.gather_segment_reduce(mode, t, gp, size, seg_ptr=seg_ptr,
                                                                    out_dtype=od), x, S)
            check_op(torch, lambda t, od: ops.gather_segment_reduce(mode, t, ids, size, count=count,
                                                                    out_dtype=od), x, S)
            check_op(torch, lambda t, od: ops.gather_segment_reduce(mode, t, gp.to(torch.int64), size,
                                                                    seg_ptr=seg_ptr, out_dtype=od), x, S)


def test_scatter_softmax_rounds_once(EA, torch_cuda, gen):
    torch = torch_cuda
    ops = EA.ops
    idx = torch.randint(0, 40, (600,), generator=gen, device="cuda", dtype=torch.int32)
    for S in _S(torch):
        x = draw(torch, gen, (600, 20), S)
        check_op(torch, lambda t, od: ops.scatter_("softmax", t, idx, 40, out_dtype=od), x, S)


def test_scatter_mean_of_2_pow_24_updates_falls_back(EA, torch_cuda, gen):
    """E >= 2^24: the one-pass mean is refused by the library (a count may not be an exact
    f32); scatter_mean composes scatter_add as the fp32 op does, under the same contract"""
    torch = torch_cuda
    ops = EA.ops
    S = torch.bfloat16
    e, d, size = (1 << 24) + 8, 8, 1 << 16
    x = draw(torch, gen, (e, d), S)
    idx = (torch.arange(e, device="cuda", dtype=torch.int64) * size // e).to(torch.int32)
    with pytest.raises(EA._lib.EulerGpuError):
        ops._scatter_raw(2, x, idx, size)
    want32 = ops.scatter_mean(x.float(), idx, size)
    assert same(ops.scatter_mean(x, idx, size, out_dtype=torch.float32), want32)
    assert same(ops.scatter_mean(x, idx, size), want32.to(S))


@pytest.mark.parametrize("d", [8, 20])
@pytest.mark.parametrize("which", [0, 1])
def test_gradients_are_the_fp32_gradients_rounded_once(EA, torch_cuda, gen, which, d):
    torch = torch_cuda
    S = _S(torch)[which]
    ops = EA.ops
    rows, size, count = 80, 30, 6
    e = size * count
    si = torch.randint(0, size, (e,), generator=gen, device="cuda", dtype=torch.int32)
    gi = torch.randint(0, rows, (e,), generator=gen, device="cuda", dtype=torch.int32)
    ids = gi.to(torch.int64).clone()
    ids[::11] = -1
    lens = torch.randint(0, 9, (size,), generator=gen, device="cuda")
    seg_ptr = torch.zeros(size + 1, dtype=torch.int64, device="cuda")
    seg_ptr[1:] = torch.cumsum(lens, 0)
    gp = torch.randint(0, rows, (int(seg_ptr[-1]),), generator=gen, device="cuda", dtype=torch.int32)
    cases = [("gather", rows, lambda t, od: ops.gather(t, gi, out_dtype=od))]
    for mode in MODES + ["softmax"]:
        cases.append(("scatter_" + mode, e, lambda t, od, m=mode: ops.scatter_(m, t, si, size, out_dtype=od)))
    for mode in MODES:
        cases.append(("gather_scatter_" + mode, rows,
                      lambda t, od, m=mode: ops.gather_scatter(m, t, gi, si, size, out_dtype=od)))
        cases.append(("segment_count_" + mode, rows,
                      lambda t, od, m=mode: ops.gather_segment_reduce(m, t, gi, size, count=count, out_dtype=od)))
        cases.append(("segment_ids_" + mode, rows,
                      lambda t, od, m=mode: ops.gather_segment_reduce(m, t, ids, size, count=count, out_dtype=od)))
        cases.append(("segment_ptr_" + mode, rows,
                      lambda t, od, m=mode: ops.gather_segment_reduce(m, t, gp, size, seg_ptr=seg_ptr,
                                                                      out_dtype=od)))
    for name, n_in, fn in cases:
        x = draw(torch, gen, (n_in, d), S)
        x32 = x.float().requires_grad_(True)
        out32 = fn(x32, None)
        for od in (S, torch.float32):                       # grad arrives in 16 bits / as fp32
            g = draw(torch, gen, tuple(out32.shape), od if od != torch.float32 else S).to(od)
            xs = x.clone().requires_grad_(True)
            out = fn(xs, od)
            assert out.dtype == od
            out.backward(g)
            x32.grad = None
            out32.backward(g.float(), retain_graph=True)
            assert xs.grad.dtype == S
            assert same(xs.grad, x32.grad.to(S)), (name, od)


def _uniform_graph(EA, O, n=4000, seed=3):
    rng = np.random.default_rng(seed)
    ids = np.arange(10, 10 + n).astype(np.uint64)
    seg = np.arange(n + 1, dtype=np.int64) * 3
    csr = O.csr_from_raw(ids, seg, rng.choice(ids, 3 * n), np.ones(3 * n, np.float32), 1)
    val = (rng.random((n, 232)) * 8 - 4).astype(np.float32)          # slots of 100, 128 and 4 values
    feats = (3, np.arange(n + 1, dtype=np.int64) * 232, np.tile(np.array([104, 232, 232], np.int32), n),
             val.reshape(-1))

    def make():
        return EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w,
                                 csr.type_prefix, csr.n_types, csr.node_type, csr.node_weight,
                                 features=feats)
    return make, ids, val.size


def _feature_battery(torch, make, q, fids, dims, S, table_elems=None):
    G32, G = make(), make()
    before = [o.clone() for o in G32.get_dense_feature(q, fids, dims)]
    assert all(o.dtype == torch.float32 for o in before)
    # an fp32 table serves 16-bit rows, rounded once at the store
    for o, w in zip(G32.get_dense_feature(q, fids, dims, out_dtype=S), before):
        assert same(o, w.to(S))
    assert G.dense_feature_dtype == torch.float32
    b0 = G.device_bytes
    G.set_dense_feature_dtype(S)
    assert G.dense_feature_dtype == S
    b1 = G.device_bytes
    assert b1 < b0
    if table_elems is not None:
        assert b0 - b1 == 2 * table_elems               # 4 bytes an element -> 2
    G.set_dense_feature_dtype(S)                        # a second call is a no-op
    assert G.device_bytes == b1 and G.dense_feature_dtype == S
    with pytest.raises(ValueError):
        G.set_dense_feature_dtype(torch.float32)        # the bits are gone
    other = torch.float16 if S == torch.bfloat16 else torch.bfloat16
    with pytest.raises(ValueError):
        G.set_dense_feature_dtype(other)
    with pytest.raises(TypeError):
        G.get_dense_feature(q, fids, dims, out_dtype=other)
    with pytest.raises(TypeError):
        G.set_dense_feature_dtype(torch.float64)
    for o, w in zip(G.get_dense_feature(q, fids, dims, out_dtype=torch.float32), before):
        assert same(o, w.to(S).float())
    for od in (S, None):
        for o, w in zip(G.get_dense_feature(q, fids, dims, out_dtype=od), before):
            assert same(o, w.to(S))
    return G32, G, before


@pytest.mark.parametrize("which", [0, 1])
def test_ragged_feature_table_in_16_bits(EA, O, torch_cuda, fixture_csr, which):
    torch = torch_cuda
    S = _S(torch)[which]
    fg = np.load(os.path.join(ROOT, "tests", "golden", "features.npz"))
    q = torch.as_tensor(np.concatenate([fg["fx_query"], [0, 10 ** 9]]).astype(np.int64)).cuda()
    n_float = int(fg["fx_n_float"])
    fids = list(range(n_float)) * 3 + [n_float + 2, -1]          # every slot; two that do not exist
    dims = [1] * n_float + [3] * n_float + [40] * n_float + [5, 5]     # shorter and longer than stored
    _, _, before = _feature_battery(
        torch, lambda: EA.Graph.load(os.path.join(ROOT, "tests", "golden", "fixture_dat")), q, fids, dims, S)
    assert any(o.any() for o in before)
    assert not before[-1].any() and not before[-2].any()          # unknown slots: zeros
    assert all(not o[-2:].any() for o in before)                  # unknown ids: zero rows
    feats = (n_float, fg["fx_feat_ptr"], fg["fx_feat_idx"], fg["fx_feat_val"])
    csr = fixture_csr
    _feature_battery(
        torch, lambda: EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w,
                                         csr.type_prefix, csr.n_types, csr.node_type, csr.node_weight,
                                         features=feats),
        q, fids, dims, S, table_elems=int(fg["fx_feat_val"].size) if fg["fx_feat_val"].size >= 8 else None)


@pytest.mark.parametrize("which", [0, 1])
def test_uniform_feature_table_in_16_bits(EA, O, torch_cuda, which):
    torch = torch_cuda
    S = _S(torch)[which]
    make, ids, elems = _uniform_graph(EA, O)
    rng = np.random.default_rng(8)
    q = torch.as_tensor(np.concatenate([rng.choice(ids, 5000), [0, 3, 10 ** 9]]).astype(np.int64)).cuda()
    # slot 0 holds 104 values, slot 1 128 (both begin at multiples of 8: 16-byte lanes when dim
    # % 8 == 0, the element kernel for dims 100 and 20), slot 2 none
    fids = [0, 0, 0, 1, 1, 1, 1, 2, 5]
    dims = [100, 128, 104, 128, 64, 136, 20, 8, 8]
    G32, G, before = _feature_battery(torch, make, q, fids, dims, S, table_elems=elems)
    assert all(not o[-3:].any() for o in before) and not before[-1].any() and not before[-2].any()
    # an output row that is 2-byte but not 16-byte aligned takes the element kernel: same rows
    # (through the raw entry: the tensor API always hands over aligned rows)
    n = q.numel()
    buf = torch.zeros(n * 128 + 8, dtype=S, device="cuda")
    L = EA._lib.lib()
    code = {torch.bfloat16: 1, torch.float16: 2}[S]
    EA._lib.check(L.euler_gpu_get_dense_feature_t(G._h, None, C.c_void_p(q.data_ptr()), n, 1, 128,
                                                  C.c_void_p(buf.data_ptr() + 2), code))
    torch.cuda.synchronize()
    assert same(buf[1:1 + n * 128].view(n, 128), before[3].to(S))
    # sample_fanout_with_feature: the fp32 graph's features, rounded
    roots = q[:600]
    for g in (G32, G):
        g.set_seed(5)
    nb32, _, _, dense32 = G32.sample_fanout_with_feature(roots, [[0], [0]], [3, 2], -1, [0, 1], [100, 128],
                                                         call_id=9)
    for od in (None, S, torch.float32):
        nb, _, _, dense = G.sample_fanout_with_feature(roots, [[0], [0]], [3, 2], -1, [0, 1], [100, 128],
                                                       call_id=9, out_dtype=od)
        assert all(torch.equal(a, b) for a, b in zip(nb, nb32))
        assert len(dense) == len(dense32) == 6
        for o, w in zip(dense, dense32):
            assert same(o, w.to(S) if od != torch.float32 else w.to(S).float())
    nb, _, _, dense = G32.sample_fanout_with_feature(roots, [[0], [0]], [3, 2], -1, [0, 1], [100, 128],
                                                     call_id=9, out_dtype=S)
    for o, w in zip(dense, dense32):
        assert same(o, w.to(S))
    # the operator surface
    from euler_amd import euler_ops
    from euler_amd.euler_ops import base as _base
    prev = _base._default
    _base.set_default_graph(G)
    try:
        got = euler_ops.get_dense_feature(q, ["1"], [128])[0]
        assert same(got, before[3].to(S))
        got = euler_ops.get_dense_feature(q, ["1"], [128], out_dtype=torch.float32)[0]
        assert same(got, before[3].to(S).float())
    finally:
        _base._default = prev


def test_errors(EA, O, torch_cuda, gen):
    torch = torch_cuda
    ops = EA.ops
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    for bad in (torch.zeros((4, 8), dtype=torch.float64, device="cuda"),
                torch.zeros((4, 8), dtype=torch.int32, device="cuda"),
                torch.zeros((4, 8), dtype=torch.int64, device="cuda")):
        for call in (lambda t: ops.gather(t, idx), lambda t: ops.scatter_add(t, idx, 2),
                     lambda t: ops.scatter_max(t, idx, 2), lambda t: ops.scatter_mean(t, idx, 2),
                     lambda t: ops.scatter_("softmax", t, idx, 2),
                     lambda t: ops.gather_scatter("add", t, idx, idx, 2),
                     lambda t: ops.gather_segment_reduce("mean", t, idx, 2, count=2)):
            with pytest.raises(TypeError):
                call(bad)
    xb = torch.zeros((4, 8), dtype=torch.bfloat16, device="cuda")
    xf = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    for x, od in ((xb, torch.float16), (xf, torch.bfloat16), (xb, torch.float64)):
        with pytest.raises(TypeError):
            ops.scatter_add(x, idx, 2, out_dtype=od)
        with pytest.raises(TypeError):
            ops.gather(x, idx, out_dtype=od)
    # the raw C entries: EULER_GPU_EINVAL and a last-error text
    L = EA._lib.lib()
    out = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    calls = [
        lambda i, o: L.euler_gpu_gather_t(None, p(xb), i, p(idx), 4, 8, 4, p(out), o),
        lambda i, o: L.euler_gpu_scatter_t(None, 0, p(xb), i, p(idx), 4, 8, 2, p(out), o),
        lambda i, o: L.euler_gpu_gather_scatter_t(None, 0, p(xb), i, p(idx), p(idx), 4, 8, 2, p(out), o),
        lambda i, o: L.euler_gpu_gather_segment_reduce_t(None, 0, p(xb), i, p(idx), None, 2, 8, 2, p(out), o),
    ]
    for call in calls:
        for i, o, text in ((7, 0, b"unknown dtype"), (-1, 0, b"unknown dtype"), (1, 2, b"out_dtype"),
                           (0, 1, b"out_dtype"), (2, 5, b"out_dtype")):
            assert call(i, o) == EA._lib.EINVAL
            assert text in L.euler_gpu_last_error()
    make, ids, _ = _uniform_graph(EA, O, n=64)
    G = make()
    assert L.euler_gpu_graph_set_dense_feature_dtype(G._h, None, 9) == EA._lib.EINVAL
    assert b"unknown dtype" in L.euler_gpu_last_error()
    q = torch.as_tensor(ids[:4].astype(np.int64)).cuda()
    assert L.euler_gpu_get_dense_feature_t(G._h, None, p(q), 4, 0, 8, p(out), 4) == EA._lib.EINVAL
    assert b"unknown dtype" in L.euler_gpu_last_error()
    G.set_dense_feature_dtype(torch.bfloat16)
    assert L.euler_gpu_get_dense_feature_t(G._h, None, p(q), 4, 0, 8, p(out), 2) == EA._lib.EINVAL
    assert b"out_dtype" in L.euler_gpu_last_error()
    assert L.euler_gpu_graph_set_dense_feature_dtype(G._h, None, 0) == EA._lib.EINVAL
    # a graph without dense features has nothing to convert
    G0 = EA.Graph.synthetic(EA.synth_params(1, 2000, 20000, weighted=True))
    with pytest.raises(ValueError):
        G0.set_dense_feature_dtype(torch.bfloat16)


def test_autocast_sage_mean_forward_and_backward(EA, torch_cuda):
    """Two SAGE-mean layers over sage_blocks of the fixture graph under bf16 autocast: the model
    on the 16-bit ops equals, bit for bit, the same model written with the fp32 ops on widened
    inputs and one rounding per aggregation - activations, loss and every parameter gradient."""
    torch = torch_cuda
    from euler_amd.dataflow import SageDataFlow
    ops = EA.ops
    G = EA.Graph.load(os.path.join(ROOT, "tests", "golden", "fixture_dat"))
    G.set_seed(11)
    max_id = int(G.id_range()[0])
    flow = SageDataFlow(G, [4, 3], [[0, 1], [0, 1]], add_self_loops=True, max_id=max_id)
    roots = torch.arange(1, min(max_id, 6) + 1, device="cuda", dtype=torch.int64)
    df = flow(roots)
    blocks = list(df)
    torch.manual_seed(3)
    d_in, d_h = 24, 16
    feat = (torch.rand((max_id + 2, d_in), device="cuda") * 2 - 1)
    lins = [torch.nn.Linear(d_in, d_h).cuda(), torch.nn.Linear(d_h, 8).cuda()]

    def agg_half(h, blk):
        assert h.dtype == torch.bfloat16
        return ops.gather_scatter("mean", h, blk.edge_index[1], blk.edge_index[0], blk.size[0])

    def agg_wide(h, blk):
        return ops.gather_scatter("mean", h.float(), blk.edge_index[1], blk.edge_index[0],
                                  blk.size[0]).to(torch.bfloat16)

    def run(agg):
        for lin in lins:
            lin.zero_grad()
        acts = []
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            h = feat[blocks[0].n_id]
            for blk, lin in zip(blocks, lins):
                h = torch.relu(agg(lin(h), blk))
                acts.append(h)
            loss = (h.float() ** 2).sum()
        loss.backward()
        return acts, loss.detach(), [p.grad.clone() for lin in lins for p in lin.parameters()]

    acts_h, loss_h, grads_h = run(agg_half)
    acts_w, loss_w, grads_w = run(agg_wide)
    assert acts_h[-1].shape[0] == roots.numel() and acts_h[-1].dtype == torch.bfloat16
    for a, b in zip(acts_h, acts_w):
        assert same(a, b)
    assert same(loss_h.reshape(1), loss_w.reshape(1)) and float(loss_h) > 0
    for a, b in zip(grads_h, grads_w):
        assert a.abs().sum() > 0 and same(a, b)
