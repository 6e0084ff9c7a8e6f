"""tests/mp_base_ref.py is what the GPU tests of the fp32 base ops are measured against, so it is
checked here without a GPU: its forward against the oracle's sequential loops bit for bit, its
float64 gradient formulas against torch's CPU autograd in float64 on index_add_ / index_select /
scatter_reduce(amax).  The inputs of the gradient checks are small integers, so that ties (2-way,
3-way, more) occur and every float64 operation of either side is exact or rounded alike."""
import numpy as np
import pytest
import torch

import mp_base_ref as R

MODES = ["add", "max", "mean"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("e,d,size,sort", [(900, 5, 40, False), (700, 8, 33, True), (1, 3, 4, False),
                                           (300, 1, 300, False)])
def test_forward_equals_the_oracle(O, e, d, size, sort):
    rng = np.random.default_rng(e + d)
    x = (rng.standard_normal((e, d)) * 10.0 ** rng.uniform(-3, 3, (e, d))).astype(np.float32)
    keys = rng.integers(0, size, e).astype(np.int32)
    keys[keys == 2] = 3                                     # an empty destination
    if sort:
        keys = np.sort(keys)
    assert same_bits(R.scatter_ref("add", x, keys, size), O.scatter_add(x, keys, size))
    assert same_bits(R.scatter_ref("max", x, keys, size), O.scatter_max(x, keys, size))
    assert same_bits(R.scatter_ref("mean", x, keys, size), O.scatter_mean(x, keys, size))
    table = rng.standard_normal((size, d)).astype(np.float32)
    assert same_bits(R.gather_ref(table, keys), O.gather(table, keys))
    gi = rng.integers(0, size, e).astype(np.int32)
    assert same_bits(R.gather_scatter_ref("add", table, gi, keys, size), O.scatter_add(O.gather(table, gi), keys, size))
    # keys outside [0, size) are left out: the same result as without those updates
    wide = keys.copy()
    wide[::7] = -1 - (np.arange(len(wide[::7])) % 3)
    wide[3::11] = size + (np.arange(len(wide[3::11])) % 4)
    ok = R.valid_keys(wide, size)
    assert not ok.all() or e == 1
    for op, oracle in (("add", O.scatter_add), ("max", O.scatter_max), ("mean", O.scatter_mean)):
        assert same_bits(R.scatter_ref(op, x, wide, size), oracle(x[ok], wide[ok], size))


def test_forward_edges():
    x = np.array([[1.0, -2e9], [2.0, -3e9]], np.float32)
    keys = np.array([1, 1], np.int32)
    assert R.scatter_ref("add", x, keys, 3).tolist() == [[0, 0], [3.0, float(np.float32(-2e9) + np.float32(-3e9))], [0, 0]]
    assert R.scatter_ref("max", x, keys, 3).tolist() == [[-1e9, -1e9], [2.0, -1e9], [-1e9, -1e9]]
    assert same_bits(R.scatter_ref("mean", x, keys, 3)[1, :1], np.float32([3.0]) / (np.float32(2) + np.float32(1e-7)))
    assert R.segment_keys(3, count=2).tolist() == [0, 0, 1, 1, 2, 2]
    assert R.segment_keys(3, seg_ptr=[0, 2, 2, 3]).tolist() == [0, 0, 2]
    assert R.id_rows([-1, 3, 9, (1 << 33) + 2, 10], 10).tolist() == [9, 3, 9, 2, 9]
    assert R.mean_denominator([0, 1, 3]).dtype == np.float32


def _case(seed, sort):
    rng = np.random.default_rng(seed)
    e, d, size, rows = 400, 5, 23, 31
    keys = rng.integers(-2, size + 2, e)
    keys[keys == 4] = 5
    if sort:
        keys = np.sort(keys)
    x = rng.integers(0, 4, (e, d)).astype(np.float64)          # small set: ties
    table = rng.integers(0, 4, (rows, d)).astype(np.float64)
    gi = rng.integers(0, rows - 2, e)                           # rows that nothing reads
    g = rng.integers(-8, 9, (size, d)).astype(np.float64)
    return e, d, size, rows, keys, x, table, gi, g


def _torch_scatter(op, src, keys, size):
    """float64 torch CPU form of the op on the updates with a destination"""
    k = torch.as_tensor(keys, dtype=torch.int64)
    d = src.shape[1]
    if op == "max":
        init = torch.full((size, d), R.INIT["max"], dtype=torch.float64)
        return init.scatter_reduce(0, k.reshape(-1, 1).expand(-1, d), src, "amax", include_self=True)
    out = torch.zeros((size, d), dtype=torch.float64).index_add_(0, k, src)
    if op == "mean":
        cnt = np.bincount(keys, minlength=size)
        out = out / torch.as_tensor(R.mean_denominator(cnt).astype(np.float64)).reshape(-1, 1)
    return out


@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("op", MODES)
def test_scatter_gradients_equal_torch_float64(op, sort):
    e, d, size, rows, keys, x, table, gi, g = _case(11, sort)
    ok = R.valid_keys(keys, size)
    assert 0 < ok.sum() < e
    src = torch.tensor(x[ok], requires_grad=True)
    _torch_scatter(op, src, keys[ok], size).backward(torch.as_tensor(g))
    want = np.zeros((e, d))
    want[ok] = src.grad.numpy()                                  # left-out updates: 0
    got = R.edge_terms(op, x, g, keys, size)
    assert got.dtype == np.float64
    if op == "max":      # (1 / n) * g here, as mp_ops.py:61-62 has it; torch divides g by n
        assert np.allclose(got, want, rtol=4e-16, atol=0) and np.array_equal(got == 0, want == 0)
    else:
        assert np.array_equal(got, want)
    if op == "add":                                              # a copy keeps the dtype of g
        g32 = g.astype(np.float32)
        assert same_bits(R.scatter_add_grad(g32, keys), want.astype(np.float32))
    if op == "max":
        is_max, n_max = R.max_selected(x, keys, size)
        assert {2, 3, 4} <= set(np.unique(n_max[is_max]).tolist())
        assert not is_max[~ok].any()


@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("op", MODES)
def test_gather_scatter_gradient_equals_torch_float64(op, sort):
    e, d, size, rows, keys, x, table, gi, g = _case(12, sort)
    ok = R.valid_keys(keys, size)
    t = torch.tensor(table, requires_grad=True)
    src = t.index_select(0, torch.as_tensor(gi[ok]))
    _torch_scatter(op, src, keys[ok], size).backward(torch.as_tensor(g))
    want, mag, m = R.gather_scatter_grad(op, table, gi, g, keys, size)
    # integers and, for mean / max, quotients summed in another order: exact for add, else close
    if op == "add":
        assert np.array_equal(want, t.grad.numpy())
    else:
        assert np.allclose(want, t.grad.numpy(), rtol=1e-13, atol=1e-13)
    assert np.array_equal(m, np.bincount(gi, minlength=rows)) and (m[-2:] == 0).all()
    assert (want[-2:] == 0).all() and (mag >= np.abs(want) - 1e-12).all()


def test_gather_gradient_equals_torch_float64():
    e, d, size, rows, keys, x, table, gi, g = _case(13, False)
    t = torch.tensor(table, requires_grad=True)
    ge = np.random.default_rng(5).integers(-8, 9, (e, d)).astype(np.float64)
    t.index_select(0, torch.as_tensor(gi)).backward(torch.as_tensor(ge))
    got = R.gather_grad(ge.astype(np.float32), gi, rows)          # small integers: float32 is exact
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), t.grad.numpy())
