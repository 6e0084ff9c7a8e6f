"""The fp32 base of the message-passing ops - gather, scatter_add / _max / _mean, gather_scatter and
gather_segment_reduce (GatherRowsKernel, SegmentReduceKernel, SegmentReduceVec4Kernel, the key
grouping, and the autograd Functions of euler_amd/ops.py) - against tests/mp_base_ref.py, which
is plain numpy and is itself checked on the host (test_mp_base_ref_host.py).

Forward: the bits of the sequential float32 loop per destination in input order, at every row
width that takes another path through the kernels, every segment length 0 .. 20 and a hub of 1000
updates, keys sorted and unsorted, data aligned to 16 bytes and 4 bytes into its storage, past the
cap of the grid, with keys outside [0, size) (left out) and with NaN / inf / -0.0.

Gradients, against the float64 formulas of the reference (u = 2^-24, gamma_k = k u / (1 - k u);
every bound is derived, none carries a margin):
  scatter_add, gather, gather_scatter("add") and the segment forms with add: bit-equal;
  scatter_mean: one fp32 division by the exact float32 denominator: bit-equal to the float32
    quotient (the division on the GPU is correctly rounded: see test_gradients);
  scatter_max: two roundings, |err| <= (2u + u^2) |want|; bit-equal where the number of equal
    maxima is a power of two; exactly 0 for non-maxima;
  gather_scatter / gather_segment_reduce with mean or max: |err| <= gamma_(m+2) sum |t_p| for a
    table row read by m edges with per-edge terms t_p; exactly 0 for a row that nothing reads;
  an update whose key is outside [0, size): exactly 0, whatever grad holds."""
import functools

import numpy as np
import pytest

import mp_base_ref as R

pytestmark = pytest.mark.gpu

MODES = ["add", "max", "mean"]
U = 2.0 ** -24
I32 = np.iinfo(np.int32)


def dev(torch, a, unaligned=False):
    """a numpy array in GPU memory; unaligned: a contiguous view that starts 4 bytes into its storage"""
    t = torch.tensor(np.ascontiguousarray(a), device="cuda")
    if unaligned:
        assert t.element_size() == 4
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        buf[1:] = t.reshape(-1)
        t = buf[1:].view(t.shape)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def same_bits(got, want):
    """got (a GPU tensor) has the dtype, the shape and the bits of want (float32 numpy or tensor)"""
    import torch
    if isinstance(want, np.ndarray):
        assert want.dtype == np.float32
        want = torch.tensor(want, device=got.device)
    if got.dtype != torch.float32 or got.shape != want.shape:
        return False
    return torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


def same_bits_or_nan(got, want):
    """NaN where want is NaN (its sign and payload are not specified), the bits of want elsewhere"""
    got = got.detach().cpu().numpy()
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


# ---- forward -----------------------------------------------------------------------------------
SIZE, ROWS, HUB, COUNT = 67, 301, 40, 13      # 67 destinations: no multiple of any rows_per_block
DIMS = [1, 3, 4, 8, 12, 16, 32, 64, 100, 128, 256, 260, 512]
# Vec4 (d % 4 == 0, d / 4 divides 64): 4 .. 256, rows_per_wave 64 .. 1; 12 and 260 are multiples of
# 4 that are not Vec4; 512 has d / 4 > 64; 100, 260, 512: the scalar kernel's column loop (d > 64)


@functools.lru_cache(maxsize=None)
def sweep_keys():
    """the key column of the sweep: every segment length 0 .. 20 (the 8 / 4 / 1 tails, exactly 8 and
    16), one hub, empty destinations at rows 0 and SIZE - 1; the gather rows and ids that go with it"""
    rng = np.random.default_rng(2024)
    lens = rng.integers(0, 21, SIZE)
    lens[1:22] = np.arange(21)
    lens[HUB] = 1000
    lens[0] = lens[SIZE - 1] = 0
    srt = np.repeat(np.arange(SIZE), lens).astype(np.int32)
    e = len(srt)
    uns = srt[rng.permutation(e)]
    assert set(np.bincount(uns, minlength=SIZE).tolist()) >= set(range(21)) and (np.diff(uns) < 0).any()
    gi = rng.integers(0, ROWS, e).astype(np.int32)
    ids = gi.astype(np.int64)
    ids[::13] = -1                                            # default_node: the last row
    ids[3::17] = ROWS + np.arange(len(ids[3::17])) * 7        # past the table: the last row
    ids[5::19] += 1 << 33                                     # only the low word counts
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return dict(zip(("sorted", "unsorted", "gi", "ids", "ptr"), frozen(srt, uns, gi, ids, ptr)), e=e)


@functools.lru_cache(maxsize=None)
def sweep_case(d):
    """(table [ROWS, d], updates = table[gi], the expected outputs) - computed once per width"""
    k = sweep_keys()
    rng = np.random.default_rng(100 + d)
    # magnitudes over six decades: a sum in another order has other bits
    table = (rng.standard_normal((ROWS, d)) * 10.0 ** rng.uniform(-3, 3, (ROWS, d))).astype(np.float32)
    upd = R.gather_ref(table, k["gi"])
    ne = SIZE * COUNT
    rows = R.id_rows(k["ids"], ROWS)
    assert (rows != k["gi"]).any() and rows.max() == ROWS - 1
    by_count = R.segment_keys(SIZE, count=COUNT)
    want = {}
    for op in MODES:
        want[op, "unsorted"] = R.scatter_ref(op, upd, k["unsorted"], SIZE)
        want[op, "sorted"] = R.scatter_ref(op, upd, k["sorted"], SIZE)
        want[op, "count"] = R.scatter_ref(op, upd[:ne], by_count, SIZE)
        want[op, "ids_ptr"] = R.scatter_ref(op, table[rows], k["sorted"], SIZE)
        want[op, "ids_count"] = R.scatter_ref(op, table[rows[:ne]], by_count, SIZE)
    for order in ("unsorted", "sorted"):
        hub = upd[np.flatnonzero(k[order] == HUB)]
        assert len(hub) == 1000
        assert not np.array_equal(R.reduce_rows("add", hub, d), R.reduce_rows("add", hub[::-1], d))
    frozen(table, upd, *want.values())
    return table, upd, want


@pytest.mark.parametrize("d", DIMS)
def test_forward_sweep(EA, torch_cuda, d):
    torch, ops = torch_cuda, EA.ops
    k = sweep_keys()
    table, upd, want = sweep_case(d)
    ne = SIZE * COUNT
    keys = {order: dev(torch, k[order]) for order in ("unsorted", "sorted")}
    gi, ids, ptr = dev(torch, k["gi"]), dev(torch, k["ids"]), dev(torch, k["ptr"])
    assert gi.dtype == torch.int32 and ids.dtype == torch.int64 and ptr.dtype == torch.int64
    for unaligned in (False, True):
        x, t = dev(torch, upd, unaligned), dev(torch, table, unaligned)
        why = (d, unaligned)
        assert same_bits(ops.gather(t, gi), upd), why
        for op in MODES:
            for order in ("unsorted", "sorted"):
                assert same_bits(ops.scatter_(op, x, keys[order], SIZE), want[op, order]), (op, order, why)
                assert same_bits(ops.gather_scatter(op, t, gi, keys[order], SIZE), want[op, order]), (op, order, why)
            assert same_bits(ops.gather_segment_reduce(op, t, gi[:ne], SIZE, count=COUNT), want[op, "count"]), (op, why)
            assert same_bits(ops.gather_segment_reduce(op, t, gi, SIZE, seg_ptr=ptr), want[op, "sorted"]), (op, why)
            assert same_bits(ops.gather_segment_reduce(op, t, ids, SIZE, seg_ptr=ptr), want[op, "ids_ptr"]), (op, why)
            assert same_bits(ops.gather_segment_reduce(op, t, ids[:ne], SIZE, count=COUNT),
                             want[op, "ids_count"]), (op, why)


@pytest.mark.parametrize("d", [3, 8, 64])
def test_keys_outside_the_range_are_left_out(EA, torch_cuda, d):
    torch, ops = torch_cuda, EA.ops
    k = sweep_keys()
    table, upd, _ = sweep_case(d)
    rng = np.random.default_rng(d)
    wide = k["unsorted"].copy()
    at = rng.choice(k["e"], 160, replace=False)
    wide[at[:70]] = -1 - rng.integers(0, 5, 70)
    wide[at[70:140]] = SIZE + rng.integers(0, 5, 70)
    wide[at[140:150]] = I32.min
    wide[at[150:]] = I32.max
    x, t, gi = dev(torch, upd), dev(torch, table), dev(torch, k["gi"])
    for keys in (wide, np.sort(wide)):
        ok = R.valid_keys(keys, SIZE)
        assert (keys[~ok] < 0).any() and (keys[~ok] >= SIZE).any()
        kt = dev(torch, keys)
        for op in MODES:
            want = R.scatter_ref(op, upd, keys, SIZE)
            assert np.array_equal(want, R.scatter_ref(op, upd[ok], keys[ok], SIZE))
            assert (want[[0, SIZE - 1]] == np.float32(R.INIT[op])).all()          # 0, -1e9, 0
            assert same_bits(ops.scatter_(op, x, kt, SIZE), want), (op, d)
            assert same_bits(ops.gather_scatter(op, t, gi, kt, SIZE), want), (op, d)


# The segment reduces launch at most 8192 blocks of (64, 4) threads and loop beyond that; a block
# covers 4 rows (scalar kernel) or 4 * 64 / (d / 4) rows (Vec4).  (d, destinations):
GRID = [(3, 40_000), (256, 40_000), (4, 600_000), (16, 600_000), (4, 2_200_000)]
GRID_BLOCKS = 8192


def rows_per_block(d):
    vec4 = d % 4 == 0 and d // 4 <= 64 and 64 % (d // 4) == 0
    return 4 * (64 // (d // 4)) if vec4 else 4


def test_the_grid_cases_pass_the_cap():
    for d in {d for d, _ in GRID}:
        assert max(size for dd, size in GRID if dd == d) > GRID_BLOCKS * rows_per_block(d)


@pytest.mark.parametrize("d,size", GRID)
def test_grid_stride_loops(EA, torch_cuda, d, size):
    """Every destination has 0, 1 or 2 updates, so their order cannot matter and the expected
    output is vectorised numpy: the first update, or fl(first + second) / max(first, second)."""
    torch, ops = torch_cuda, EA.ops
    rng = np.random.default_rng(d + size)
    lens = rng.integers(0, 3, size)
    lens[-1], lens[-2], lens[-3] = 2, 0, 1                   # non-empty destinations in the last pass
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    e = int(ptr[-1])
    u = rng.standard_normal((e, d), dtype=np.float32)
    first, second = u[np.minimum(ptr[:-1], e - 1)], u[np.minimum(ptr[:-1] + 1, e - 1)]
    n = lens[:, None]
    add = np.where(n == 0, np.float32(0), np.where(n == 1, first, first + second))
    want = {"add": add,
            "max": np.where(n == 0, np.float32(R.INIT["max"]), np.where(n == 1, first, np.maximum(first, second))),
            "mean": add / R.mean_denominator(lens)[:, None]}
    want = {op: dev(torch, w) for op, w in want.items()}
    keys = np.repeat(np.arange(size), lens).astype(np.int32)
    perm = rng.permutation(e)
    x, kt = dev(torch, u), dev(torch, keys)
    xp, kp = x[dev(torch, perm)], dev(torch, keys[perm])
    every = torch.arange(e, device="cuda", dtype=torch.int32)
    pt = dev(torch, ptr)
    for op in MODES:
        assert same_bits(ops.scatter_(op, x, kt, size), want[op]), op
        assert same_bits(ops.scatter_(op, xp, kp, size), want[op]), op
        assert same_bits(ops.gather_segment_reduce(op, x, every, size, seg_ptr=pt), want[op]), op


@pytest.mark.parametrize("d,e,unaligned", [(3, 350_000, False), (4, 1_050_000, False), (4, 263_000, True)])
def test_gather_grid_stride_loop(EA, torch_cuda, d, e, unaligned):
    """gather launches at most 4096 blocks of 256 threads (GridFor), one float or float4 each"""
    torch, ops = torch_cuda, EA.ops
    per_thread = 4 if d % 4 == 0 and not unaligned else 1
    assert e * d // per_thread > 4096 * 256
    rng = np.random.default_rng(e)
    table = rng.standard_normal((1000, d), dtype=np.float32)
    idx = rng.integers(0, 1000, e).astype(np.int32)
    assert same_bits(ops.gather(dev(torch, table, unaligned), dev(torch, idx)), R.gather_ref(table, idx))


@pytest.mark.parametrize("d", [3, 4])
def test_special_values(EA, O, torch_cuda, d):
    """NaN, +-inf and -0.0 among the updates: whatever the oracle's sequential loop gives"""
    torch, ops = torch_cuda, EA.ops
    rng = np.random.default_rng(77 + d)
    size, e = 7, 90                                           # destination 6 stays empty
    keys = rng.permutation(np.arange(e) % (size - 1)).astype(np.int32)       # 15 updates each
    u = rng.standard_normal((e, d)).astype(np.float32)
    at = [np.flatnonzero(keys == r) for r in range(size)]
    assert all(len(p) >= 9 for p in at[:6])                   # the eight-wide loop and a tail
    u[at[0][1], 0] = np.nan                                   # a NaN between finite updates
    u[at[1][0], 0], u[at[1][-1], 0] = np.inf, -np.inf         # inf + -inf
    u[at[1][2], 1] = np.inf
    u[at[2]] = -2e9 - np.arange(len(at[2]), dtype=np.float32)[:, None]      # all below -1e9
    u[at[3], 0] = -0.0                                        # only -0.0 in a column
    u[at[3][4], 1] = -np.inf
    u[at[4][0]] = np.nan                                      # NaN first and last
    u[at[4][-1]] = np.nan
    u[at[5][3], 2] = -0.0
    order = np.argsort(keys, kind="stable")
    oracle = {"add": O.scatter_add, "max": O.scatter_max, "mean": O.scatter_mean}
    back = np.arange(e - 1, -1, -1).astype(np.int32)          # the updates as rows of a table, reversed
    table = dev(torch, u[::-1])
    for kk, uu, gi in ((keys, u, back), (keys[order], u[order], back[order])):
        x, kt, git = dev(torch, uu), dev(torch, kk), dev(torch, gi)
        for op in MODES:
            want = oracle[op](uu, kk, size)
            assert np.isnan(want).any() or op == "max"
            assert same_bits_or_nan(ops.scatter_(op, x, kt, size), want), (op, d)
            assert same_bits_or_nan(ops.gather_scatter(op, table, git, kt, size), want), (op, d)
        assert (oracle["max"](uu, kk, size)[2] == np.float32(-1e9)).all()


def test_plumbing(EA, torch_cuda):
    torch, ops = torch_cuda, EA.ops
    rng = np.random.default_rng(5)
    e, d, size, rows = 50, 6, 9, 14
    table = rng.standard_normal((rows, d)).astype(np.float32)
    gi = rng.integers(0, rows, e)
    keys = rng.integers(0, size, e)
    u = R.gather_ref(table, gi)
    named = {"add": ops.scatter_add, "max": ops.scatter_max, "mean": ops.scatter_mean}
    x, k32, g32 = dev(torch, u), dev(torch, keys.astype(np.int32)), dev(torch, gi.astype(np.int32))
    k64, g64 = dev(torch, keys.astype(np.int64)), dev(torch, gi.astype(np.int64))
    xt, tt = dev(torch, u.T).t(), dev(torch, table.T).t()     # transposed views of [d, e] / [d, rows]
    assert not xt.is_contiguous() and not tt.is_contiguous() and xt.shape == (e, d)
    assert same_bits(ops.gather(tt, g64), u)
    for op in MODES:
        want = R.scatter_ref(op, u, keys, size)
        assert same_bits(named[op](x, k32, size), want)       # scatter_(name, ...) is the named op
        assert same_bits(ops.scatter_(op, x, k32, size), want)
        assert same_bits(ops.scatter_(op, xt, k64, size), want)
        assert same_bits(ops.gather_scatter(op, tt, g64, k64, size), want)
        init = np.full((size, d), R.INIT[op], np.float32)
        none = torch.empty(0, dtype=torch.int32, device="cuda")
        assert same_bits(ops.scatter_(op, torch.empty((0, d), device="cuda"), none, size), init)      # E = 0
        assert same_bits(ops.gather_scatter(op, dev(torch, table), none, none, size), init)
        assert ops.scatter_(op, x, k32, 0).shape == (0, d)                                            # size = 0
        assert ops.gather_scatter(op, dev(torch, table), g32, k32, 0).shape == (0, d)
        assert ops.scatter_(op, torch.empty((e, 0), device="cuda"), k32, size).shape == (size, 0)     # D = 0
        assert same_bits(ops.scatter_(op, x[:1], k32[:1], size), R.scatter_ref(op, u[:1], keys[:1], size))   # E = 1
    assert ops.gather(dev(torch, table), torch.empty(0, dtype=torch.int32, device="cuda")).shape == (0, d)
    assert ops.gather(torch.empty((rows, 0), device="cuda"), g32).shape == (e, 0)
    assert same_bits(ops.gather(dev(torch, table), g32[:1]), u[:1])


# ---- gradients ---------------------------------------------------------------------------------
G_SIZE, G_ROWS, G_E, G_COUNT = 41, 97, 500, 12
G_DIMS = [3, 8, 20, 64]
FORMS = ["scatter_add", "scatter_max", "scatter_mean", "gather", "gather_scatter", "count", "ptr", "ids"]


@functools.lru_cache(maxsize=None)
def grad_case(d, ties):
    """ties: every value from {0, 1, 2, 3}, so that a segment has 2, 3 and 4 equal maxima in a column
    (and other columns hold the same values: ties across columns must not count)"""
    rng = np.random.default_rng(7 + d + 1000 * ties)
    keys = rng.integers(-3, G_SIZE + 3, G_E).astype(np.int32)       # some keys < 0 and >= size
    keys[keys == 5] = 6                                             # empty destinations
    keys[keys == G_SIZE - 1] = 0
    keys[np.flatnonzero(keys == 9)[1:]] = 10                        # exactly one update: the only count
    assert (keys == 9).sum() == 1                                   # at which fl(cnt + 1e-7) != cnt
    gi = rng.integers(0, G_ROWS - 3, G_E).astype(np.int32)          # repeated rows; three that nothing reads
    if ties:
        table = rng.integers(0, 4, (G_ROWS, d)).astype(np.float32)
    else:
        table = (rng.standard_normal((G_ROWS, d)) * 4).astype(np.float32)
    g = rng.standard_normal((G_SIZE, d)).astype(np.float32)
    ge = rng.standard_normal((G_E, d)).astype(np.float32)
    lens = rng.integers(0, 25, G_SIZE)
    lens[::7] = 0
    lens[1] = 1
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert ptr[-1] <= G_E
    ids = gi.astype(np.int64)
    ids[::11] = -1
    ids[4::23] = G_ROWS + 3
    ids[6::29] += 1 << 35
    return frozen(keys, gi, table, g, ge, ptr, ids)


def grad_twice(torch, fn, x, g):
    """the gradient of fn at x for the output gradient g; two runs give equal bits"""
    out = []
    for _ in range(2):
        a = x.clone().requires_grad_(True)
        out.append(torch.autograd.grad(fn(a), a, g)[0])
    assert same_bits(out[0], out[1])
    return out[0]


def ulp32(w):
    """one unit in the last place of float32 at the float64 values w"""
    return np.ldexp(1.0, np.maximum(np.frexp(np.abs(w))[1] - 1, -126) - 23)


def check_table_grad(op, got, table, rows, g, keys, size):
    """the gradient of reduce(op, table[rows], keys, size) with respect to table"""
    if op == "add":       # exact copies of g's rows (0 for a left-out update) summed in input order
        assert same_bits(got, R.gather_grad(R.scatter_add_grad(g, keys), rows, table.shape[0])), op
        return
    want, mag, m = R.gather_scatter_grad(op, table, rows, g, keys, size)
    k = (m + 2.0)[:, None]
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    assert (err <= k * U / (1 - k * U) * mag).all(), (op, float((err - k * U / (1 - k * U) * mag).max()))
    assert (m == 0).any() and (got.cpu().numpy()[m == 0] == 0).all()


@pytest.mark.parametrize("d", G_DIMS)
@pytest.mark.parametrize("form", FORMS)
def test_gradients(EA, torch_cuda, form, d):
    """scatter_mean: one fp32 division of grad by fl(count + 1e-7).  Measured on an MI355X: torch's
    fp32 division there is correctly rounded - the gradient is bit-equal to numpy's float32 quotient
    at every width, sorted and unsorted - so equality is what is asserted (and with it half an ulp
    of fp32 at the float64 value), not the 1 ulp that a division by reciprocal would need."""
    torch, ops = torch_cuda, EA.ops
    for ties in ((False,) if form in ("gather", "scatter_add") else (False, True)):
        keys0, gi, table, g, ge, ptr, ids = grad_case(d, ties)
        gt, tt, git = dev(torch, g), dev(torch, table), dev(torch, gi)
        if form == "gather":
            got = grad_twice(torch, lambda t: ops.gather(t, git), tt, dev(torch, ge))
            assert same_bits(got, R.gather_grad(ge, gi, G_ROWS))
            continue
        if form in ("count", "ptr", "ids"):
            if form == "count":
                kw, n, keys = dict(count=G_COUNT), G_SIZE * G_COUNT, R.segment_keys(G_SIZE, count=G_COUNT)
            else:
                kw, n, keys = dict(seg_ptr=dev(torch, ptr)), int(ptr[-1]), R.segment_keys(G_SIZE, seg_ptr=ptr)
            index = dev(torch, ids[:n]) if form == "ids" else git[:n]
            rows = R.id_rows(ids[:n], G_ROWS) if form == "ids" else gi[:n]
            if form == "ids":     # an id outside the table sends its gradient to the last row
                assert (rows == G_ROWS - 1).any() and (gi != G_ROWS - 1).all()
            for op in MODES:
                got = grad_twice(torch, lambda t: ops.gather_segment_reduce(op, t, index, G_SIZE, **kw), tt, gt)
                check_table_grad(op, got, table, rows, g, keys, G_SIZE)
            continue
        for keys in (keys0, np.sort(keys0)):
            ok = R.valid_keys(keys, G_SIZE)
            assert (keys[~ok] < 0).any() and (keys[~ok] >= G_SIZE).any()
            kt = dev(torch, keys)
            if form == "gather_scatter":
                for op in MODES:
                    got = grad_twice(torch, lambda t: ops.gather_scatter(op, t, git, kt, G_SIZE), tt, gt)
                    check_table_grad(op, got, table, gi, g, keys, G_SIZE)
                continue
            x = R.gather_ref(table, gi)
            got_t = grad_twice(torch, lambda a: getattr(ops, form)(a, kt, G_SIZE), dev(torch, x), gt)
            got = got_t.cpu().numpy()
            assert (got[~ok] == 0).all()
            if form == "scatter_add":
                assert same_bits(got_t, R.scatter_add_grad(g, keys))
            elif form == "scatter_mean":
                want = R.scatter_mean_grad(g, keys, G_SIZE)
                cnt = np.bincount(keys[ok], minlength=G_SIZE)
                quotient = R.scatter_add_grad((g / R.mean_denominator(cnt)[:, None]).astype(np.float32), keys)
                assert same_bits(got_t, quotient)
                assert (np.abs(got.astype(np.float64) - want) <= 0.5 * ulp32(want)).all()
            else:
                want = R.scatter_max_grad(x, g, keys, G_SIZE)
                is_max, n_max = R.max_selected(x, keys, G_SIZE)
                if ties:
                    assert {2, 3, 4} <= set(np.unique(n_max[is_max]).tolist())
                assert (np.abs(got.astype(np.float64) - want) <= (2 * U + U * U) * np.abs(want)).all()
                assert (got[~is_max] == 0).all()
                pow2 = is_max & ((n_max & (n_max - 1)) == 0)            # an exact fraction: one rounding
                product = (np.float32(1) / n_max.astype(np.float32)) * R.scatter_add_grad(g, keys)
                assert np.array_equal(got.view(np.int32)[pow2], product.view(np.int32)[pow2])


@pytest.mark.parametrize("which", [0, 1, 2])
def test_updates_without_a_destination_get_zero_gradient(EA, torch_cuda, which):
    """Keys < 0 and >= size (INT32_MIN and INT32_MAX among them) in every keyed op, with and without
    edge_weight, fp32 and 16-bit: the gradient of such an update is exactly 0 and the other gradients
    have the bits they have without those updates - although grad is NaN in row 0, the row a key
    made safe by clamping would read (destination 0 is empty)."""
    torch, ops = torch_cuda, EA.ops
    S = [torch.float32, torch.bfloat16, torch.float16][which]
    rng = np.random.default_rng(31)
    e, d, heads, size, rows = 240, 8, 2, 20, 30
    keys = rng.integers(1, size, e).astype(np.int32)
    at = rng.choice(e, 80, replace=False)
    keys[at[:35]] = -1 - rng.integers(0, 4, 35)
    keys[at[35:70]] = size + rng.integers(0, 4, 35)
    keys[at[70:75]] = I32.min
    keys[at[75:]] = I32.max
    g = rng.standard_normal((size, d)).astype(np.float32)
    g[0] = np.nan
    gt = dev(torch, g)
    table = dev(torch, rng.integers(0, 4, (rows, d)).astype(np.float32)).to(S)     # ties for max
    w = dev(torch, (rng.standard_normal((e, heads)) + 3).astype(np.float32))
    gi_np = rng.integers(0, rows, e).astype(np.int32)

    def grads(fn, *inputs):
        leaves = [t.clone().requires_grad_(True) for t in inputs]
        return torch.autograd.grad(fn(*leaves), leaves, gt)

    def equal(a, b):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16 if a.element_size() == 2
                                                                                else torch.int32),
                                                                         b.view(torch.int16 if b.element_size() == 2
                                                                                else torch.int32))

    for order in (np.arange(e), np.argsort(keys, kind="stable")):
        kk, gg = keys[order], gi_np[order]
        ok = R.valid_keys(kk, size)
        assert 0 < (~ok).sum() and (kk[ok] != 0).all()
        kt, git, okt = dev(torch, kk), dev(torch, gg), dev(torch, ok)
        kf, gf = kt[okt], git[okt]
        x = ops.gather(table, git).detach()
        for op in MODES:
            (gx,) = grads(lambda a: ops.scatter_(op, a, kt, size, out_dtype=torch.float32), x)
            (gx_f,) = grads(lambda a: ops.scatter_(op, a, kf, size, out_dtype=torch.float32), x[okt])
            assert gx.dtype == S and bool((gx[~okt] == 0).all()) and equal(gx[okt], gx_f), (op, S)
            (gp,) = grads(lambda t: ops.gather_scatter(op, t, git, kt, size, out_dtype=torch.float32), table)
            (gp_f,) = grads(lambda t: ops.gather_scatter(op, t, gf, kf, size, out_dtype=torch.float32), table)
            assert not bool(torch.isnan(gp.float()).any()) and equal(gp, gp_f), (op, S)
            gp, gw = grads(lambda t, ww: ops.gather_scatter(op, t, git, kt, size, out_dtype=torch.float32,
                                                            edge_weight=ww), table, w)
            gp_f, gw_f = grads(lambda t, ww: ops.gather_scatter(op, t, gf, kf, size, out_dtype=torch.float32,
                                                                edge_weight=ww), table, w[okt])
            assert not bool(torch.isnan(gp.float()).any()) and equal(gp, gp_f), (op, S)
            assert bool((gw[~okt] == 0).all()) and equal(gw[okt], gw_f), (op, S)
