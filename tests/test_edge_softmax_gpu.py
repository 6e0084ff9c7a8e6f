"""ops.edge_softmax on the GPU.
A. Bit equality, no tolerance: the fp32 op equals the numpy restatement tests/edge_softmax_ref.py
   through all three segment forms; unsorted keys equal sorted ones after the permutation; the
   forms agree; two calls agree; 16-bit storage is the fp32 op on the widened input, rounded once;
   autograd returns the bits of the raw _grad entry.
B. Accuracy against float64 with the derived bounds of edge_softmax_ref (no margin); the error of
   the device's torch.exp on the subsample is recorded beside E (nothing is asserted about it) and
   takes E's place in the bound of the scatter_softmax composition."""
import ctypes as C

import numpy as np
import pytest
import torch

import edge_softmax_ref as ref

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().cpu().contiguous().view(-1).view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a) == bits(b)).all())


def same_np(t, a):
    got = t.detach().cpu().numpy()
    return got.dtype == a.dtype == np.float32 and got.shape == a.shape and \
        np.array_equal(got.view(np.uint32), a.view(np.uint32))


def power_law_ptr(rng, size, hub):
    """segment lengths: many empty and short ones, some past 32 and past 256, and one hub"""
    lens = np.minimum((rng.pareto(1.1, size) * 3).astype(np.int64), 3000)
    lens[rng.random(size) < 0.2] = 0
    lens[size // 3] = hub
    lens[0] = 0
    lens[-1] = 0
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def block_logits(rng, e, heads):
    x = (rng.standard_normal((e, heads)) * 4).astype(np.float32)
    far = rng.random(e) < 0.01
    x[far] -= np.float32(100.0)                   # differences to the maximum beyond T: flushed
    x[rng.random(e) < 0.002] = -np.inf
    return x


def run_forms(torch, ops, x, sp_np, size, g=None):
    """the op (or, with g, the raw gradient entry on y = x) through seg_ptr, sorted keys and
    unsorted keys; returns the three results in GROUPED order"""
    dev = "cuda"
    e = x.shape[0]
    lens = sp_np[1:] - sp_np[:-1]
    keys = np.repeat(np.arange(size, dtype=np.int32), lens)
    sp = torch.as_tensor(sp_np, device=dev)
    k = torch.as_tensor(keys, device=dev)
    # a shuffle that keeps the order of the updates INSIDE a destination (the stable sort of the
    # unsorted path restores exactly the grouped order): slot j holds grouped update perm[j]
    slot_keys = keys[np.random.default_rng(e).permutation(e)]
    perm = np.empty(e, np.int64)
    perm[np.argsort(slot_keys, kind="stable")] = np.arange(e)
    inv = torch.as_tensor(perm, device=dev)

    def call(t, gg, **kw):
        if gg is None:
            return ops.edge_softmax(t, **kw)
        return ops._edge_softmax_raw(t.contiguous(), gg.contiguous(), kw.get("indices"), kw.get("seg_ptr"), 0,
                                     size, torch.float32)
    by_ptr = call(x, g, seg_ptr=sp, size=size)
    by_keys = call(x, g, indices=k, size=size)
    xs = torch.empty_like(x)
    xs[:] = x[inv]
    gs = None if g is None else g[inv].contiguous()
    shuffled = call(xs, gs, indices=k[inv].contiguous(), size=size)
    back = torch.empty_like(shuffled)
    back[inv] = shuffled
    return by_ptr, by_keys, back


@pytest.mark.parametrize("heads", [1, 4, 3])
def test_uniform_count_block_equals_the_restatement(EA, torch_cuda, heads):
    torch, ops = torch_cuda, EA.ops
    for count, size in ((10, 3000), (25, 1111), (32, 200), (33, 150), (700, 37)):
        rng = np.random.default_rng(count * 7 + heads)
        x_np = block_logits(rng, size * count, heads)
        x_np[::count] = np.where(np.isfinite(x_np[::count]), x_np[::count], 0)      # a finite maximum
        sp_np = np.arange(size + 1, dtype=np.int64) * count
        want = ref.edge_softmax_ref(x_np, sp_np)
        x = torch.as_tensor(x_np, device="cuda")
        got = ops.edge_softmax(x, count=count, size=size)
        assert same_np(got, want), (count, size)
        assert same(got, ops.edge_softmax(x, count=count))                      # run to run, size implied
        by_ptr, by_keys, back = run_forms(torch, ops, x, sp_np, size)
        assert same(got, by_ptr) and same(got, by_keys) and same(got, back)
        assert bool((got[torch.isneginf(x)] == 0).all())
        g_np = rng.standard_normal((size * count, heads)).astype(np.float32)
        g = torch.as_tensor(g_np, device="cuda")
        want_g = ref.edge_softmax_ref(want, sp_np, g_np)
        raw = ops._edge_softmax_raw(got, g, None, None, count, size, torch.float32)
        assert same_np(raw, want_g), (count, size)
        a, b, c = run_forms(torch, ops, got, sp_np, size, g)
        assert same(raw, a) and same(raw, b) and same(raw, c)
        if heads == 1:                                                          # [E] and [E, 1]
            flat = ops.edge_softmax(x[:, 0].contiguous(), count=count)
            assert flat.shape == (size * count,) and same(flat, got[:, 0].contiguous())


@pytest.mark.parametrize("heads", [1, 8])
def test_power_law_block_with_empty_segments_and_a_hub(EA, torch_cuda, heads):
    torch, ops = torch_cuda, EA.ops
    rng = np.random.default_rng(heads)
    size, hub = 5000, 100_003
    sp_np = power_law_ptr(rng, size, hub)
    lens = sp_np[1:] - sp_np[:-1]
    assert lens.max() >= 100_000 and (lens == 0).sum() > 500 and ((lens > 32) & (lens <= 256)).any()
    e = int(sp_np[-1])
    x_np = block_logits(rng, e, heads)
    x_np[sp_np[:-1][lens > 0]] = 1.0                                         # a finite maximum everywhere
    want = ref.edge_softmax_ref(x_np, sp_np)
    x = torch.as_tensor(x_np, device="cuda")
    by_ptr, by_keys, back = run_forms(torch, ops, x, sp_np, size)
    assert same_np(by_ptr, want)
    assert same(by_ptr, by_keys) and same(by_ptr, back)
    assert same(by_ptr, ops.edge_softmax(x, seg_ptr=torch.as_tensor(sp_np, device="cuda")))
    # contract B, forward
    err = np.abs(by_ptr.cpu().numpy().astype(np.float64) - ref.forward_f64(x_np, sp_np))
    bound = ref.forward_bound(x_np, sp_np, ref.E_ULP)
    print("forward: largest error / bound = %.4f" % float((err / bound).max()))
    assert np.all(err <= bound)
    g_np = (rng.standard_normal((e, heads)) * 3).astype(np.float32)
    g = torch.as_tensor(g_np, device="cuda")
    a, b, c = run_forms(torch, ops, by_ptr, sp_np, size, g)
    assert same_np(a, ref.edge_softmax_ref(want, sp_np, g_np))
    assert same(a, b) and same(a, c)
    err = np.abs(a.cpu().numpy().astype(np.float64) - ref.backward_f64(want, g_np, sp_np))
    bound = ref.backward_bound(want, g_np, sp_np)
    print("backward: largest error / bound = %.4f" % float((err[bound > 0] / bound[bound > 0]).max()))
    assert np.all(err <= bound)


def test_out_of_range_keys_get_zero(EA, torch_cuda):
    torch, ops = torch_cuda, EA.ops
    rng = np.random.default_rng(17)
    size, e, heads = 50, 4000, 2
    keys = rng.integers(-5, size + 7, e).astype(np.int32)
    keys[:40] = 7                                                            # (one segment past 32)
    x_np = (rng.standard_normal((e, heads)) * 3).astype(np.float32)
    order = np.argsort(keys, kind="stable")
    inside = (keys[order] >= 0) & (keys[order] < size)
    sp_np = ref.seg_ptr_of_sorted_keys(keys[order], size)
    want = np.zeros_like(x_np)
    want[order] = ref.edge_softmax_ref(x_np[order], sp_np)
    x = torch.as_tensor(x_np, device="cuda")
    k = torch.as_tensor(keys, device="cuda")
    x.requires_grad_(True)
    got = ops.edge_softmax(x, indices=k, size=size)
    assert same_np(got, want)
    assert bool((got.detach().cpu().numpy()[order][~inside] == 0).all()) and (~inside).sum() > 100
    g_np = rng.standard_normal((e, heads)).astype(np.float32)
    got.backward(torch.as_tensor(g_np, device="cuda"))
    want_g = np.zeros_like(x_np)
    want_g[order] = ref.edge_softmax_ref(want[order], sp_np, g_np[order])
    assert same_np(x.grad, want_g)
    assert bool((x.grad.cpu().numpy()[order][~inside] == 0).all())
    # sorted keys with the same outsiders
    ks = torch.as_tensor(keys[order], device="cuda")
    assert same_np(ops.edge_softmax(torch.as_tensor(x_np[order], device="cuda"), indices=ks, size=size),
                   want[order])


@pytest.mark.parametrize("heads", [1, 3])
def test_updates_outside_the_span_of_seg_ptr_get_zero(EA, torch_cuda, heads):
    """seg_ptr need not start at 0 or end at e: what lies outside it belongs to no destination and
    gets output 0 and gradient 0, as edge_softmax_ref says - never what the buffer held."""
    torch, ops = torch_cuda, EA.ops
    rng = np.random.default_rng(41 + heads)
    lens = np.array([0, 9, 40, 0, 3, 300, 0], np.int64)
    for lead, trail in ((37, 55), (0, 20), (13, 0)):
        sp_np = lead + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        e = int(sp_np[-1]) + trail
        x_np = (rng.standard_normal((e, heads)) * 3).astype(np.float32)
        g_np = rng.standard_normal((e, heads)).astype(np.float32)
        want = ref.edge_softmax_ref(x_np, sp_np)
        assert np.all(want[:lead] == 0) and np.all(want[e - trail:] == 0)
        x = torch.as_tensor(x_np, device="cuda")
        sp = torch.as_tensor(sp_np, device="cuda")
        for S in (torch.float32, torch.bfloat16):
            # (dirty memory of the same size first: the allocator hands it to the next output)
            dirty = torch.full((e, heads), 7.0, device="cuda", dtype=S)
            del dirty
            xr = x.to(S).clone().requires_grad_(True)
            y = ops.edge_softmax(xr, seg_ptr=sp)
            if S == torch.float32:
                assert same_np(y, want)
            assert bool((y[:lead] == 0).all()) and bool((y[e - trail:] == 0).all())
            dirty = torch.full((e, heads), 7.0, device="cuda", dtype=S)
            del dirty
            y.backward(torch.as_tensor(g_np, device="cuda").to(S))
            if S == torch.float32:
                assert same_np(xr.grad, ref.edge_softmax_ref(want, sp_np, g_np))
            assert bool((xr.grad[:lead] == 0).all()) and bool((xr.grad[e - trail:] == 0).all())
    # no destination at all: everything is outside
    y = ops.edge_softmax(x, seg_ptr=torch.tensor([5], device="cuda"))
    assert bool((y == 0).all())


def test_a_nan_logit_gets_zero_in_short_and_long_segments(EA, torch_cuda):
    """outside the contract, documented: the NaN is left out of the maximum wherever it stands"""
    torch, ops = torch_cuda, EA.ops
    rng = np.random.default_rng(43)
    for n in (10, 32, 33, 700):
        x_np = (rng.standard_normal((n * 3, 2)) * 3).astype(np.float32)
        x_np[0, 0] = x_np[n + n // 2, 0] = x_np[3 * n - 1, 0] = np.nan        # first, middle, last
        y = ops.edge_softmax(torch.as_tensor(x_np, device="cuda"), count=n).cpu().numpy()
        nan = np.isnan(x_np)
        assert np.all(y[nan].view(np.uint32) == 0) and np.all(np.isfinite(y))
        assert np.allclose(y.reshape(3, n, 2).astype(np.float64).sum(axis=1), 1.0, rtol=0, atol=1e-5)


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
def test_16_bit_storage_is_the_fp32_op_rounded_once(EA, torch_cuda, dt):
    torch, ops = torch_cuda, EA.ops
    S = getattr(torch, dt)
    rng = np.random.default_rng(3)
    size, heads = 700, 4
    sp_np = power_law_ptr(rng, size, 4000)
    e = int(sp_np[-1])
    x = torch.as_tensor((rng.standard_normal((e, heads)) * 4).astype(np.float32), device="cuda").to(S)
    sp = torch.as_tensor(sp_np, device="cuda")
    y32 = ops.edge_softmax(x.float(), seg_ptr=sp)
    assert same(ops.edge_softmax(x, seg_ptr=sp, out_dtype=torch.float32), y32)
    assert same(ops.edge_softmax(x, seg_ptr=sp), y32.to(S))
    assert same(ops.edge_softmax(x, seg_ptr=sp, out_dtype=S), y32.to(S))
    # the backward: fp32 arithmetic on the saved fp32 output, one rounding to the input's dtype
    g32 = torch.as_tensor(rng.standard_normal((e, heads)).astype(np.float32), device="cuda")
    raw = ops._edge_softmax_raw(y32, g32, None, sp, 0, size, torch.float32)
    for od, g in ((torch.float32, g32), (None, g32.to(S))):
        xr = x.clone().requires_grad_(True)
        out = ops.edge_softmax(xr, seg_ptr=sp, out_dtype=od)
        assert out.dtype == (torch.float32 if od is not None else S)
        out.backward(g)
        want = raw if od is not None else ops._edge_softmax_raw(y32, g.float(), None, sp, 0, size, torch.float32)
        assert xr.grad.dtype == S and same(xr.grad, want.to(S))
        # a 16-bit g is widened exactly by the kernel
        if od is None:
            assert same(ops._edge_softmax_raw(y32, g, None, sp, 0, size, torch.float32), want)


def test_autograd_returns_the_bits_of_the_grad_entry(EA, torch_cuda):
    torch, ops = torch_cuda, EA.ops
    rng = np.random.default_rng(23)
    size, count, heads = 900, 10, 8
    x = torch.as_tensor(rng.standard_normal((size * count, heads)).astype(np.float32), device="cuda")
    g = torch.as_tensor(rng.standard_normal((size * count, heads)).astype(np.float32), device="cuda")
    xr = x.clone().requires_grad_(True)
    y = ops.edge_softmax(xr, count=count, size=size)
    y.backward(g)
    assert same(xr.grad, ops._edge_softmax_raw(y.detach(), g, None, None, count, size, torch.float32))
    # the rows of a softmax sum to one, so a constant gradient per destination gives (nearly) none
    xr.grad = None
    ops.edge_softmax(xr, count=count, size=size).backward(torch.ones_like(g))
    assert float(xr.grad.abs().max()) < 1e-6


def test_fused_and_composed_lie_within_the_bound_of_float64(EA, torch_cuda):
    """Sanity: both are softmaxes.  The error of torch.exp on the device over the subsample is
    recorded (printed) beside E and used in the composition's bound; nothing is asserted about it."""
    torch, ops = torch_cuda, EA.ops
    d = torch.as_tensor(ref.exp_subsample().view(np.float32).copy(), device="cuda")
    e_torch = float(ref.ulp_error(torch.exp(d).cpu().numpy(), d.cpu().numpy()).max())
    print("exp error on the subsample, in ulps: torch.exp on the device %.4f; ExpNonPositive E = %.4f"
          % (e_torch, ref.E_ULP))
    rng = np.random.default_rng(29)
    size, count, heads = 2000, 25, 4
    x_np = (rng.standard_normal((size * count, heads)) * 6).astype(np.float32)
    sp_np = np.arange(size + 1, dtype=np.int64) * count
    x = torch.as_tensor(x_np, device="cuda")
    dst = torch.arange(size, device="cuda", dtype=torch.int32).repeat_interleave(count)
    exact = ref.forward_f64(x_np, sp_np)
    fused = ops.edge_softmax(x, count=count).cpu().numpy().astype(np.float64)
    composed = ops.scatter_softmax(x, dst, size).cpu().numpy().astype(np.float64)
    assert np.all(np.abs(fused - exact) <= ref.forward_bound(x_np, sp_np, ref.E_ULP))
    assert np.all(np.abs(composed - exact) <= ref.forward_bound(x_np, sp_np, e_torch))


def test_argument_checks(EA, torch_cuda):
    torch, ops = torch_cuda, EA.ops
    x = torch.zeros((12, 2), device="cuda")
    k = torch.zeros(12, dtype=torch.int32, device="cuda")
    sp = torch.tensor([0, 5, 12], device="cuda")
    with pytest.raises(ValueError):
        ops.edge_softmax(x)
    with pytest.raises(ValueError):
        ops.edge_softmax(x, indices=k, size=3, count=4)
    with pytest.raises(ValueError):
        ops.edge_softmax(x, indices=k)
    with pytest.raises(ValueError):
        ops.edge_softmax(x, indices=k[:5], size=3)
    with pytest.raises(ValueError):
        ops.edge_softmax(x, seg_ptr=sp, size=5)
    with pytest.raises(ValueError):
        ops.edge_softmax(x, count=5)
    with pytest.raises(ValueError):
        ops.edge_softmax(x.reshape(3, 4, 2), count=1)
    with pytest.raises(TypeError):
        ops.edge_softmax(x.double(), count=4)
    with pytest.raises(TypeError):
        ops.edge_softmax(x, count=4, out_dtype=torch.float16)
    with pytest.raises(RuntimeError):
        ops.edge_softmax(x.cpu(), count=4)
    assert ops.edge_softmax(x[:0], count=3).shape == (0, 2)
    # an empty segment writes nothing; its neighbours are whole
    y = ops.edge_softmax(x, seg_ptr=torch.tensor([0, 5, 5, 12], device="cuda"))
    assert bool((y[:5] == 0.2).all()) and bool((y[5:] == np.float32(1) / np.float32(7)).all())


def test_c_abi_error_rules(EA, torch_cuda):
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()
    EINVAL = -1
    x = torch.zeros((6, 2), device="cuda")
    out = torch.full((6, 2), 7.0, device="cuda")
    k = torch.zeros(6, dtype=torch.int32, device="cuda")
    sp = torch.tensor([0, 6], device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    f = L.euler_gpu_edge_softmax
    assert f(None, p(x), 0, p(k), None, 0, 6, 0, 1, p(out), 0) == EINVAL          # heads < 1
    assert f(None, None, 0, p(k), None, 0, 6, 2, 1, p(out), 0) == EINVAL          # null buffer
    assert f(None, p(x), 0, p(k), None, 0, 6, 2, 1, None, 0) == EINVAL
    assert f(None, p(x), 5, p(k), None, 0, 6, 2, 1, p(out), 0) == EINVAL          # unknown dtype
    assert f(None, p(x), 0, p(k), None, 0, 6, 2, 1, p(out), 1) == EINVAL          # out neither fp32 nor in
    assert f(None, p(x), 0, p(k), None, 0, 1 << 31, 2, 1, p(out), 0) == EINVAL    # e >= 2^31
    assert f(None, p(x), 0, p(k), p(sp), 0, 6, 2, 1, p(out), 0) == EINVAL         # two forms
    assert f(None, p(x), 0, p(k), None, 6, 6, 2, 1, p(out), 0) == EINVAL
    assert f(None, p(x), 0, None, None, 0, 6, 2, 1, p(out), 0) == EINVAL          # no form
    assert f(None, p(x), 0, None, None, 4, 6, 2, 1, p(out), 0) == EINVAL          # e != size * count
    gfn = L.euler_gpu_edge_softmax_grad
    assert gfn(None, p(x), 0, None, 0, p(k), None, 0, 6, 2, 1, p(out), 0) == EINVAL
    assert gfn(None, p(x), 0, p(x), 9, p(k), None, 0, 6, 2, 1, p(out), 0) == EINVAL
    assert f(None, None, 0, p(k), None, 0, 0, 2, 1, None, 0) == 0                 # e == 0: nothing touched
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert f(None, p(x), 0, None, None, 6, 6, 2, 1, p(out), 0) == 0
    torch.cuda.synchronize()
    assert bool((out == np.float32(1) / np.float32(6)).all())
