"""The fused supervised loss head on the GPU (ops.supervise_loss, Graph.supervise_loss,
metrics.Streaming, euler_gpu_supervise_loss[_grad]):
  A  forward bits, counts and histograms == the numpy restatement tests/supervise_ref.py (shapes
     around the tile and partial boundaries, dtypes, unaligned views, logits at 0 and +-88)
  B  the graph form on a written feature table == the tensor form fed get_dense_feature's rows
  C  gradient bits == the restatement; autograd within the derived bound of the float64 composition
  D  streaming across calls, reset, value() without a host wait, replay from a captured graph
  E  the rules of the C entries; empty shapes; guard words
  F  the example's fused / composed agreement on the fixture graph"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import dat_write
import supervise_ref as ref

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "golden", "fixture_dat")
BS, CS = (0, 1, 63, 64, 65, 257), (1, 3, 41, 121)
TS = (None, 3, 5, 5000)
F = np.float32


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def dtypes(torch):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def unaligned(torch, x):
    """the same values in a view that starts ONE ELEMENT into its storage"""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device="cuda")
    buf[1:] = x.reshape(-1)
    out = buf[1:].view(x.shape)
    assert out.data_ptr() % 16 == x.element_size() and out.is_contiguous()
    return out


def draw(torch, rng, b, c, S, Z, kind="mix"):
    """logits of dtype S with 0, +-88 and a tiny negative planted, labels of dtype Z: hard, with
    soft ones (multiples of 1/8: exact in every dtype) among them unless kind is "ones" / "zeros" """
    x = (rng.normal(size=(b, c)) * 3).astype(F)
    flat = x.reshape(-1)
    flat[::7], flat[3::11], flat[5::13], flat[1::17] = 0, 88, -88, -1e-7
    if kind == "zero_logits":
        flat[:] = 0
    z = (rng.random((b, c)) < 0.4).astype(F)
    if kind == "ones":
        z[:] = 1
    elif kind == "zeros":
        z[:] = 0
    else:
        z.reshape(-1)[::5] = rng.integers(0, 9, z.reshape(-1)[::5].size) / 8.0
    return torch.from_numpy(x).cuda().to(S), torch.from_numpy(z).cuda().to(Z)


def widened(t):
    return t.float().cpu().numpy()


def same_f32(got, want):
    got, want = got.cpu().numpy(), np.asarray(want)
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


def bits(torch, t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def raw(torch, x, z, t=None, counts=None, hist=None, graph=None, nodes=None, fid=0, prob=True, diff=True):
    """one call of the C entry through ops._supervise_loss_raw -> dict of its outputs"""
    from euler_amd import ops
    counts = torch.zeros(5, dtype=torch.int64, device="cuda") if counts is None else counts
    if t is not None and hist is None:
        hist = torch.zeros((2, t + 1), dtype=torch.int64, device="cuda")
    loss, p, d, row_loss = ops._supervise_loss_raw(x, z, graph, nodes, fid, counts, hist if t is not None else None,
                                                   t or 0, prob, diff)
    return dict(loss=loss, prob=p, diff=d, row_loss=row_loss, counts=counts, hist=hist)


def check(torch, got, want, tag, t):
    for k in ("prob", "diff", "row_loss"):
        assert same_f32(got[k], want[k]), tag + (k,)
    assert same_f32(got["loss"], np.array([want["loss"]], F)), tag + ("loss",)
    assert np.array_equal(got["counts"].cpu().numpy(), want["counts"]), tag + ("counts",)
    if t is not None:
        assert np.array_equal(got["hist"].cpu().numpy(), want["hist"]), tag + ("hist",)


# ---- A: forward bits -------------------------------------------------------------------------
@pytest.mark.parametrize("S", ["f32", "bf16", "f16"])
def test_forward_has_the_bits_of_the_restatement(torch, S):
    """B in {0, 1, 63, 64, 65, 257} x C in {1, 3, 41, 121}: one and several tiles of both tile
    shapes, one and two column chunks, B across the 256 partials; the label dtype and T rotate"""
    from euler_amd import ops
    rng = np.random.default_rng(11)
    names = list(dtypes(torch))
    i = names.index(S)
    for b in BS:
        for c in CS:
            i += 1
            Z, t = dtypes(torch)[names[i % 3]], TS[i % 4]
            x, z = draw(torch, rng, b, c, dtypes(torch)[S], Z)
            want = ref.forward(widened(x), widened(z), t)
            check(torch, raw(torch, x, z, t), want, (S, b, c, t), t)
            out = ops.supervise_loss(x, z, return_prob=True)
            assert out[0].shape == () and same_f32(out[0].reshape(1), np.array([want["loss"]], F))
            assert same_f32(out[1], want["prob"])
    assert float(ops.supervise_loss(x[:0], z[:0])) == 0.0


@pytest.mark.parametrize("S", ["f32", "bf16", "f16"])
def test_unaligned_views(torch, S):
    rng = np.random.default_rng(12)
    for b, c in ((65, 41), (257, 3)):
        x, z = draw(torch, rng, b, c, dtypes(torch)[S], dtypes(torch)[S])
        want = ref.forward(widened(x), widened(z), 5)
        check(torch, raw(torch, unaligned(torch, x), unaligned(torch, z), 5), want, (S, b, c), 5)


@pytest.mark.parametrize("t", [3, 5, 5000])
@pytest.mark.parametrize("kind", ["zero_logits", "ones", "zeros"])
def test_counts_and_histograms_at_the_edges(torch, t, kind):
    """logits 0: p is exactly 0.5, a threshold of T = 3 and 5 (strictly below: it is not counted);
    all-positive and all-negative labels: one histogram row stays empty"""
    rng = np.random.default_rng(t)
    x, z = draw(torch, rng, 65, 41, torch.float32, torch.float32, kind)
    want = ref.forward(widened(x), widened(z), t)
    got = raw(torch, x, z, t)
    check(torch, got, want, (kind, t), t)
    hist = got["hist"].cpu().numpy()
    assert hist.sum() == 65 * 41
    assert np.array_equal(hist, np.stack([np.bincount(ref.bucket_brute(want["prob"][widened(z) != 0], t), minlength=t + 1),
                                          np.bincount(ref.bucket_brute(want["prob"][widened(z) == 0], t), minlength=t + 1)]))
    if kind == "zero_logits":
        assert hist.sum(0)[-(-(t - 1) // 2)] == 65 * 41                 # thr_i < 0.5 for i < (t - 1) / 2
        assert got["counts"].cpu().numpy()[[0, 1]].sum() == 65 * 41       # floor(0.5 + 0.5) = 1 everywhere
    if kind == "ones":
        assert hist[1].sum() == 0
    if kind == "zeros":
        assert hist[0].sum() == 0


# ---- B: the graph form -----------------------------------------------------------------------
LABEL_C = 4


@pytest.fixture(scope="module")
def label_graph(tmp_path_factory):
    """40 nodes, three float slots: 0 the features (5), 1 ragged and SHORTER than C (1 .. 3), 2 LONGER (7)"""
    rng = np.random.default_rng(21)
    ids = np.arange(40) * 3 + 5
    floats = []
    for i in range(40):
        hard = (rng.random(7) < 0.5).astype(F)
        hard[i % 7] = rng.integers(0, 9) / 8.0                            # a soft label, exact in 16 bits
        floats.append([rng.normal(size=5).astype(F), hard[:1 + i % 3], hard])
    d = tmp_path_factory.mktemp("supervise_dat")
    dat_write.write_feature_dat_dir(d, ids, floats, partitions=2)
    return str(d), ids


@pytest.mark.parametrize("table", ["f32", "bf16", "f16"])
def test_graph_form_equals_the_tensor_form(torch, label_graph, table):
    import euler_amd
    path, ids = label_graph
    G = euler_amd.Graph.load(path)
    G.set_dense_feature_dtype(dtypes(torch)[table])
    rng = np.random.default_rng(22)
    q = np.concatenate([ids, ids[::-1], [0, 987654321, 6], rng.choice(ids, 180)]).astype(np.int64)
    nodes = torch.from_numpy(q).cuda()
    b = len(q)
    x = torch.from_numpy((rng.normal(size=(b, LABEL_C)) * 3).astype(F)).cuda()
    for fid in (1, 2, 0, 9, -1):                      # shorter, longer, another slot, two unknown slots
        rows = G.get_dense_feature(nodes, [fid], [LABEL_C])[0]
        assert rows.dtype == dtypes(torch)[table]
        want = raw(torch, x, rows, 5000)
        got = raw(torch, x, None, 5000, graph=G, nodes=nodes, fid=fid)
        for k in ("prob", "diff", "row_loss", "loss"):
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (fid, k)
        assert torch.equal(got["counts"], want["counts"]) and torch.equal(got["hist"], want["hist"]), fid
        check(torch, got, ref.forward(widened(x), widened(rows), 5000), (table, fid), 5000)
        if fid in (9, -1):
            assert not bool(rows.any())
    assert bool((G.get_dense_feature(nodes, [1], [LABEL_C])[0][:, 3] == 0).all())     # zero filled past the slot
    # the public form: Graph.supervise_loss and its euler_ops twin
    from euler_amd import euler_ops, metrics
    from euler_amd.euler_ops import base
    m = metrics.Streaming("f1")
    loss, prob = G.supervise_loss(nodes, x, 2, LABEL_C, metric=m, return_prob=True)
    want = raw(torch, x, G.get_dense_feature(nodes, [2], [LABEL_C])[0])
    assert torch.equal(loss.reshape(1), want["loss"]) and torch.equal(prob, want["prob"])
    assert torch.equal(m.counts, want["counts"])
    before = base._default
    euler_ops.set_default_graph(G)
    try:
        assert torch.equal(euler_ops.supervise_loss(nodes, x, "2", LABEL_C), loss)
    finally:
        base._default = before
    with pytest.raises(ValueError):
        G.supervise_loss(nodes, x, 2, LABEL_C + 1)


# ---- C: the gradient -------------------------------------------------------------------------
UNIT = {"f32": (0.0, 0.0), "bf16": (2.0 ** -8, 0.0), "f16": (2.0 ** -11, 2.0 ** -25)}


@pytest.mark.parametrize("S", ["f32", "bf16", "f16"])
def test_gradient_bits_and_autograd(torch, S, capsys):
    """the kernel's gradient == the restatement's, rounded once to the logits' dtype; autograd
    through ops.supervise_loss against binary_cross_entropy_with_logits in float64 within the
    bound derived in supervise_ref.py plus that one rounding, no margin"""
    from euler_amd import ops
    rng = np.random.default_rng(31)
    worst = 0.0
    for b, c in ((1, 1), (65, 41), (257, 3), (64, 121)):
        x, z = draw(torch, rng, b, c, dtypes(torch)[S], torch.float32)
        x = unaligned(torch, x) if c == 41 else x
        fw = ref.forward(widened(x), widened(z))
        g = float(F(1.5 - b % 3))
        got = ops._supervise_loss_grad_raw(torch.from_numpy(fw["diff"]).cuda(), torch.tensor(g, device="cuda"),
                                           dtypes(torch)[S])
        want = torch.from_numpy(ref.grad(fw["diff"], g, b, c)).cuda().to(dtypes(torch)[S])
        assert got.dtype == want.dtype and torch.equal(bits(torch, got), bits(torch, want)), (b, c)
        xa = x.clone().requires_grad_()
        loss = ops.supervise_loss(xa, z)
        (loss * g).backward()
        assert xa.grad.dtype == x.dtype and torch.equal(bits(torch, xa.grad), bits(torch, got))
        x64 = x.double().requires_grad_()
        loss64 = torch.nn.functional.binary_cross_entropy_with_logits(x64, z.double())
        (loss64 * g).backward()
        center, bound = ref.forward64(widened(x), widened(z))
        assert abs(float(loss64.detach()) - center) <= 1e-12 * (1 + abs(center))         # the two float64 forms agree
        assert abs(float(loss.detach().double()) - float(loss64.detach())) <= bound
        gc, gb = ref.grad64(widened(x), widened(z), g, *UNIT[S])
        w64 = x64.grad.cpu().numpy()
        assert np.all(np.abs(w64 - gc) <= 1e-9 * (1e-6 + np.abs(gc)))
        err = np.abs(xa.grad.double().cpu().numpy() - w64)
        assert np.all(err <= gb), (b, c, float((err / gb).max()))
        worst = max(worst, float((err / gb).max()))
    with capsys.disabled():
        print("\n[supervise_loss %s] worst gradient error / bound %.4f" % (S, worst))
    # no gradient asked: diff is not kept; the labels never get one
    zr = z.clone().requires_grad_()
    out = ops.supervise_loss(x, zr)
    assert not out.requires_grad


# ---- D: streaming ----------------------------------------------------------------------------
def test_streaming_metrics(torch):
    from euler_amd import metrics, ops
    rng = np.random.default_rng(41)
    x, z = draw(torch, rng, 257, 41, torch.float32, torch.float32)
    whole = ref.forward(widened(x), widened(z), 5000)
    ms = {n: metrics.get(n)() for n in ("f1", "acc", "auc")}
    assert ms["auc"].num_thresholds == 5000 and metrics.get("nothing") is None
    for m in ms.values():
        ops.supervise_loss(x[:100], z[:100], metric=m)
        ops.supervise_loss(x[100:], z[100:], metric=m)                      # two calls == one on the concatenation
        assert np.array_equal(m.counts.cpu().numpy(), whole["counts"]), m.name
    assert ms["f1"].hist is None and ms["acc"].hist is None
    assert np.array_equal(ms["auc"].hist.cpu().numpy(), whole["hist"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                 # value() may not wait for the device
    try:
        values = {n: m.value() for n, m in ms.items()}
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for v in values.values():
        assert v.is_cuda and v.shape == () and v.dtype == torch.float64
    assert abs(float(values["f1"]) - ref.f1_of(whole["counts"])) <= 1e-15
    assert abs(float(values["acc"]) - ref.acc_of(whole["counts"])) <= 1e-15
    want = ref.auc_of(whole["hist"])
    assert abs(float(values["auc"]) - want) <= 1e-12 * want and 0.3 < want < 0.7
    assert abs(want - ref.auc_brute(whole["prob"], widened(z), 5000)) <= 1e-12 * want
    for m in ms.values():
        assert m.reset() is m and not bool(m.counts.any()) and (m.hist is None or not bool(m.hist.any()))
    ops.supervise_loss(x[:64], z[:64], metric=ms["auc"])
    part = ref.forward(widened(x[:64]), widened(z[:64]), 5000)
    assert np.array_equal(ms["auc"].hist.cpu().numpy(), part["hist"])
    small = metrics.Streaming("auc", num_thresholds=3, device="cuda")
    ops.supervise_loss(x, z, metric=small)
    assert np.array_equal(small.hist.cpu().numpy(), ref.forward(widened(x), widened(z), 3)["hist"])
    rank = torch.tensor([0, 1, 3], dtype=torch.int32, device="cuda")
    assert float(metrics.get("mrr")(rank)) == float(ops.rank_metric("mrr", rank))
    with pytest.raises(ValueError):
        metrics.Streaming("mrr")
    with pytest.raises(ValueError):
        metrics.Streaming("auc", num_thresholds=1)
    with pytest.raises(TypeError):
        ops.supervise_loss(x, z, metric="f1")


def test_both_entries_replay_from_a_captured_graph(torch):
    """one chain: the forward's two kernels, then the gradient kernel on the forward's diff; the
    counters and the histograms take one batch per replay"""
    from euler_amd import ops
    rng = np.random.default_rng(43)
    x, z = draw(torch, rng, 257, 41, torch.bfloat16, torch.float32)
    g = torch.tensor([0.5], device="cuda")
    want = raw(torch, x, z, 5000)
    want_g = ops._supervise_loss_grad_raw(want["diff"], g, torch.bfloat16)
    counts = torch.zeros(5, dtype=torch.int64, device="cuda")
    hist = torch.zeros((2, 5001), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = raw(torch, x, z, 5000, counts, hist)                          # (warm up)
        ops._supervise_loss_grad_raw(out["diff"], g, torch.bfloat16)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = raw(torch, x, z, 5000, counts, hist)
            out_g = ops._supervise_loss_grad_raw(out["diff"], g, torch.bfloat16)
        counts.zero_()
        hist.zero_()
        for n in (1, 2):
            for k in ("loss", "prob", "diff", "row_loss"):
                out[k].zero_()
            out_g.zero_()
            graph.replay()
            side.synchronize()
            for k in ("loss", "prob", "diff", "row_loss"):
                assert torch.equal(out[k].view(torch.int32), want[k].view(torch.int32)), k
            assert torch.equal(out_g.view(torch.int16), want_g.view(torch.int16))
            assert torch.equal(counts, n * want["counts"]) and torch.equal(hist, n * want["hist"])
    torch.cuda.current_stream().wait_stream(side)


# ---- E: the C entries ------------------------------------------------------------------------
GUARD, IGUARD = -12345.0, -777
PAD = 4                                                                  # guard words on each side


class Call(object):
    """euler_gpu_supervise_loss / _grad on small buffers with 4 guard words before and behind every output"""

    def __init__(self, torch, graph=None):
        from euler_amd import _lib
        self.torch, self.lib, self.graph = torch, _lib, graph
        self.b, self.c, self.t = 6, 3, 5
        b, c = self.b, self.c
        self.logits = torch.zeros((b, c), device="cuda")
        self.labels = torch.ones((b, c), device="cuda")
        self.nodes = torch.arange(b, device="cuda") + 1000                  # ids the graph does not have
        self.g = torch.ones(1, device="cuda")
        self.saved = torch.zeros(b * c, device="cuda")
        self.sizes = dict(prob=b * c, diff=b * c, row_loss=b, loss=1, g_logits=b * c, counts=5, hist=2 * (self.t + 1))
        self.out = {n: (torch.full((s + 2 * PAD,), IGUARD, dtype=torch.int64, device="cuda") if n in ("counts", "hist")
                        else torch.full((s + 2 * PAD,), GUARD, device="cuda")) for n, s in self.sizes.items()}

    def p(self, t, offset=0, nudge=0):
        return C.c_void_p(t.data_ptr() + t.element_size() * offset + nudge)

    def base(self):
        base = dict(logits=self.p(self.logits), logits_dt=self.lib.F32, b=self.b, c=self.c, labels=self.p(self.labels),
                    labels_dt=self.lib.F32, graph=None, nodes=None, fid=0, t=self.t, saved=self.p(self.saved),
                    g=self.p(self.g), out_dt=self.lib.F32)
        base.update({n: self.p(t, PAD) for n, t in self.out.items()})
        return base

    def graph_form(self):
        return dict(labels=None, graph=self.graph._h, nodes=self.p(self.nodes))

    def forward(self, **kw):
        from euler_amd.ops import _stream
        a = dict(self.base(), **kw)
        rc = self.lib.lib().euler_gpu_supervise_loss(
            _stream(), a["logits"], a["logits_dt"], a["b"], a["c"], a["labels"], a["labels_dt"], a["graph"], a["nodes"],
            a["fid"], a["t"], a["prob"], a["diff"], a["row_loss"], a["loss"], a["counts"], a["hist"])
        self.torch.cuda.synchronize()
        return rc

    def grad(self, **kw):
        from euler_amd.ops import _stream
        a = dict(self.base(), **kw)
        rc = self.lib.lib().euler_gpu_supervise_loss_grad(_stream(), a["saved"], a["g"], a["b"], a["c"], a["g_logits"],
                                                          a["out_dt"])
        self.torch.cuda.synchronize()
        return rc

    def guard(self, n):
        return IGUARD if n in ("counts", "hist") else GUARD

    def untouched(self, *names):
        return all(bool((self.out[n] == self.guard(n)).all()) for n in (names or self.out))

    def written(self, name, size):
        """exactly [PAD, PAD + size) was written: the guard words before and behind are intact"""
        t, gv = self.out[name], self.guard(name)
        return not bool((t[PAD:PAD + size] == gv).any()) and bool((t[:PAD] == gv).all()) and \
            bool((t[PAD + size:] == gv).all())


@pytest.fixture(scope="module")
def small_graph(label_graph):
    import euler_amd
    return euler_amd.Graph.load(label_graph[0])


def test_c_entry_error_rules(torch, small_graph):
    c = Call(torch, small_graph)
    EINVAL = c.lib.EINVAL
    fw, gr = c.forward, c.grad
    assert fw(logits_dt=3) == EINVAL and fw(logits_dt=-1) == EINVAL and fw(labels_dt=3) == EINVAL
    assert gr(out_dt=3) == EINVAL and gr(out_dt=-1) == EINVAL
    for call in (fw, gr):
        assert call(b=-1) == EINVAL and call(c=0) == EINVAL and call(c=-1) == EINVAL
        assert call(b=1 << 29, c=4) == EINVAL and call(b=1 << 31, c=1) == EINVAL and call(b=1, c=1 << 31) == EINVAL
    assert fw(t=1) == EINVAL and fw(t=0) == EINVAL and fw(t=-5) == EINVAL          # thresholds < 2 with hist given
    assert fw(graph=small_graph._h, nodes=c.p(c.nodes)) == EINVAL                   # both label forms
    assert fw(graph=small_graph._h) == EINVAL
    assert fw(labels=None) == EINVAL and fw(labels=None, nodes=c.p(c.nodes)) == EINVAL  # neither
    assert fw(**dict(c.graph_form(), nodes=None)) == EINVAL                         # the graph form without nodes
    for name in ("logits", "row_loss", "loss", "counts"):
        assert fw(**{name: None}) == EINVAL, name
    for name in ("saved", "g", "g_logits"):
        assert gr(**{name: None}) == EINVAL, name
    # a buffer not aligned to its element type
    assert fw(logits=c.p(c.logits, nudge=2)) == EINVAL and fw(labels=c.p(c.labels, nudge=2)) == EINVAL
    assert fw(logits=c.p(c.logits, nudge=1), logits_dt=c.lib.BF16) == EINVAL
    for name in ("prob", "diff", "row_loss", "loss"):
        assert fw(**{name: c.p(c.out[name], PAD, nudge=2)}) == EINVAL, name
    for name in ("counts", "hist"):
        assert fw(**{name: c.p(c.out[name], PAD, nudge=4)}) == EINVAL, name
    assert fw(**dict(c.graph_form(), nodes=c.p(c.nodes, nudge=4))) == EINVAL
    assert gr(saved=c.p(c.saved, nudge=2)) == EINVAL and gr(g=c.p(c.g, nudge=2)) == EINVAL
    assert gr(g_logits=c.p(c.out["g_logits"], PAD, nudge=2)) == EINVAL
    assert gr(g_logits=c.p(c.out["g_logits"], PAD, nudge=1), out_dt=c.lib.F16) == EINVAL
    assert c.untouched()


def test_c_entry_empty_shapes_and_guard_words(torch, small_graph):
    c = Call(torch, small_graph)
    OK = c.lib.OK
    # b == 0: the loss alone is written, +0; the counters keep their values; null buffers included
    assert c.forward(b=0) == OK and c.grad(b=0) == OK
    assert c.written("loss", 1) and float(c.out["loss"][PAD]) == 0.0 and not bool(torch.signbit(c.out["loss"][PAD]))
    assert c.untouched("prob", "diff", "row_loss", "g_logits", "counts", "hist")
    c.out["loss"].fill_(GUARD)
    assert c.forward(b=0, logits=None, labels=None, graph=small_graph._h, prob=None, diff=None, row_loss=None,
                     hist=None) == OK
    assert c.grad(b=0, saved=None, g=None, g_logits=None) == OK
    assert c.written("loss", 1) and float(c.out["loss"][PAD]) == 0.0
    # prob, diff and hist are optional
    c = Call(torch, small_graph)
    assert c.forward(prob=None, diff=None, hist=None, t=0) == OK
    assert c.untouched("prob", "diff", "hist") and c.written("row_loss", c.b) and c.written("loss", 1)
    # the full call writes exactly [B, C] / [B, C] / [B] / [1] and adds to [5] and [2][T + 1]
    for graph_form in (False, True):
        c = Call(torch, small_graph)
        form = c.graph_form() if graph_form else {}
        c.out["counts"][PAD:PAD + 5] = 100
        c.out["hist"][PAD:PAD + 2 * (c.t + 1)] = 7
        assert c.forward(**form) == OK and c.grad() == OK
        for n, s in c.sizes.items():
            assert c.written(n, s), n
        n = c.b * c.c
        # logits 0: p = 0.5, every prediction 1; tensor form: labels 1; graph form: the ids are unknown, labels 0
        want = [100 + n, 100, 100, 100 + n, 100 + n] if not form else [100, 100 + n, 100, 100, 100 + n]
        assert c.out["counts"][PAD:PAD + 5].tolist() == want
        hist = c.out["hist"][PAD:PAD + 2 * (c.t + 1)].reshape(2, c.t + 1) - 7
        assert int(hist.sum()) == n and int(hist[1 if form else 0, 2]) == n        # thr_0, thr_1 = 0.25 are below 0.5
        assert bool((c.out["g_logits"][PAD:PAD + n] == 0).all())


def test_python_argument_checks(torch):
    from euler_amd import ops
    x, z = torch.zeros((4, 3), device="cuda"), torch.ones((4, 3), device="cuda")
    with pytest.raises(ValueError):
        ops.supervise_loss(x, z[:, :2])
    with pytest.raises(ValueError):
        ops.supervise_loss(x.reshape(-1), z.reshape(-1))
    with pytest.raises(TypeError):
        ops.supervise_loss(x.double(), z)
    with pytest.raises(TypeError):
        ops.supervise_loss(x, z.long())
    with pytest.raises(RuntimeError):
        ops.supervise_loss(x.cpu(), z)
    loss, prob = ops.supervise_loss(x[:0], z[:0], return_prob=True)
    assert loss.shape == () and float(loss) == 0 and prob.shape == (0, 3)
    assert abs(float(ops.supervise_loss(x, z)) - np.log(2.0)) < 1e-6
    col = ops.supervise_loss(x.t()[:, :2], z.t()[:, :2])                      # a non-contiguous view is copied
    assert abs(float(col) - np.log(2.0)) < 1e-6


# ---- F: the example --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [[], ["--composed"]])
def test_example_trains_and_the_two_heads_agree(mode):
    """graphsage_train.py on the fixture graph: it asserts at every step that the fused and the
    composed head agree - the counts exactly, the loss within the derived bound - and that the
    loss falls"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", "graphsage_train.py"),
                        "--data", FIXTURE, "--batch", "16", "--steps", "4"] + mode,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("loss") == 4 and ("composed)" in r.stdout) == ("--composed" in mode), r.stdout
