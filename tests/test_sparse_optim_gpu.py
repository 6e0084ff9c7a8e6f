"""The fused sparse-row optimiser steps on the GPU (ops.sparse_row_step, euler_amd.optim,
euler_gpu_sparse_optim_step).  Every comparison is bit equality against the numpy restatement
tests/sparse_optim_ref.py:
  A  bits over d x E x rows x kind, the id patterns, ids that name no row, guard rows behind the
     table and the state; the count and row_index forms
  B  misaligned views of the table, the state and the gradient (V = 4 and 1); repeatability; one
     long segment; a side stream; a window past the launcher's grid cap
  C  the optimiser classes over three backward() / step() rounds, uncoalesced and coalesced
     gradients, checkpoints
  D  the refusals of Python and of the C entry, the version counters
  E  the five examples with --fused-optimizer"""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import embed_store_ref as es
import sparse_optim_ref as ref

pytestmark = pytest.mark.gpu

DIMS = [1, 3, 4, 8, 12, 64, 130, 260]
SIZES = [0, 1, 63, 64, 65, 1000]
ROWS = [1, 7, 50]
HYPER = dict(lr=0.05, momentum=0.9, betas=(0.9, 0.999))
GUARD = 0x7bcd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def tdt(torch, dt):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dt]


def dev(torch, a, dt, shift=0, extra_rows=0):
    """numpy storage (float32, or uint16 bits) -> a contiguous cuda tensor of dtype dt.  shift: the
    view starts that many elements past a 16-byte boundary; extra_rows: rows of a guard pattern
    behind the returned view, in the same allocation -> (view, guard view or None)"""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int16) if dt != "f32" else a).cuda()
    if dt != "f32":
        t = t.view(tdt(torch, dt))
    tail = extra_rows * (a.shape[1] if a.ndim == 2 else 1)
    buf = torch.empty(shift + a.size + tail, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[shift:shift + a.size].view(a.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == (shift * view.element_size()) % 16
    guard = None
    if extra_rows:
        guard = buf[shift + a.size:]
        guard.view(torch.int16 if dt != "f32" else torch.int32).fill_(GUARD)
    return view, guard


def host(torch, t):
    """a cuda tensor -> its numpy storage (float32, or uint16 bits)"""
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def guard_ok(torch, guard):
    return bool((guard.view(torch.int16 if guard.dtype != torch.float32 else torch.int32) == GUARD).all())


def stored(rng, shape, dt):
    return es.narrow(es.sensitive_values(rng, shape), dt)


def make_state(rng, kind, shape):
    """fp32 state of a kind: the accumulators of squares are positive, the others signed"""
    v = es.sensitive_values(rng, shape)
    return {"sgd": [], "momentum": [v], "adagrad": [np.abs(v)],
            "adam": [v, np.abs(es.sensitive_values(rng, shape))]}[kind]


def same_all(got, want):
    return es.same(got[0], want[0]) and len(got[1]) == len(want[1]) and all(es.same(a, b) for a, b in zip(got[1], want[1]))


def run(torch, kind, table, dt, state, ids, grad, gdt, step=1, row_index=None, count=None, shifts=(0, 0, 0)):
    """ops.sparse_row_step on device copies (shifts: of the table, the state, the gradient) ->
    (table, [state]) as numpy storage; the guard rows behind the table and the state are checked"""
    from euler_amd import ops
    t, guard = dev(torch, table, dt, shifts[0], extra_rows=1)
    st = [dev(torch, s, "f32", shifts[1], extra_rows=1) for s in state]
    g = dev(torch, grad, gdt, shifts[2])[0]
    t_ri = None if row_index is None else torch.from_numpy(np.asarray(row_index, np.int32)).cuda()
    back = ops.sparse_row_step(kind, t, torch.from_numpy(np.asarray(ids, np.int64)).cuda(), g, [s for s, _ in st],
                               step=step, row_index=t_ri, count=count, **HYPER)
    assert back is t
    assert guard_ok(torch, guard) and all(guard_ok(torch, gd) for _, gd in st)
    return host(torch, t), [host(torch, s) for s, _ in st]


def check_kind(torch, rng, kind, rows, d, ids, dt, gdt, row_index=None, count=None, step=1, shifts=(0, 0, 0), data=None):
    e = len(ids)
    m = e // count if count else (9 if row_index is not None else e)
    table, grad, state = data or (stored(rng, (rows, d), dt), stored(rng, (m, d), gdt), make_state(rng, kind, (rows, d)))
    got = run(torch, kind, table, dt, state, ids, grad, gdt, step, row_index, count, shifts)
    want = ref.step(kind, table, dt, state, ids, grad, gdt, ref.scalars(kind, step=step, **HYPER), row_index, count)
    assert same_all(got, want), (kind, rows, d, e, dt, gdt, count, row_index is not None, shifts)
    return got


# ---- A: bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_bits_of_the_restatement(torch, d):
    """every E x rows x kind; the id pattern, ids that name no row (-1, rows, 2^40, -2^63), the
    table's dtype and the gradient's dtype rotate so that every kind meets every dtype pair"""
    rng = np.random.default_rng(300 + d)
    n = 0
    for e in SIZES:
        for rows in ROWS:
            for kind in ref.KINDS:
                pattern, bad = ref.rotation(n)
                ids = es.id_pattern(rng, es.PATTERNS[pattern], rows, e)
                if bad:
                    ids = es.with_bad_ids(ids, rows)
                dt = es.DTYPES[n % 3]
                check_kind(torch, rng, kind, rows, d, ids, dt, dt if (n // 12) % 2 else "f32", step=1 + n % 5)
                n += 1


@pytest.mark.parametrize("pattern", es.PATTERNS)
def test_id_patterns(torch, pattern):
    """all distinct (rows 2000 >= E), all equal, two hubs, sorted, reverse sorted, random - with
    and without ids that name no row, every kind"""
    rng = np.random.default_rng(11)
    rows = 2000 if pattern == "distinct" else 50
    ids = es.id_pattern(rng, pattern, rows, 1000 if pattern != "equal" else 300)
    for n, kind in enumerate(ref.KINDS):
        check_kind(torch, rng, kind, rows, (4, 130)[n % 2], ids, "f32", "f32")
        check_kind(torch, rng, kind, rows, (130, 4)[n % 2], es.with_bad_ids(ids, rows), "bf16", "f32")


@pytest.mark.parametrize("kind", ref.KINDS)
def test_count_and_row_index_forms(torch, kind):
    """both forms == the restatement; a row_index entry outside [0, M) removes its occurrence"""
    rng = np.random.default_rng(31)
    rows, count = 50, 5
    for dt, d in (("f32", 12), ("bf16", 64), ("f16", 12)):
        ids = es.with_bad_ids(es.id_pattern(rng, "hubs", rows, 200 * count), rows, every=11)
        check_kind(torch, rng, kind, rows, d, ids, dt, "f32", count=count)
        ri = rng.integers(0, 9, len(ids)).astype(np.int32)
        ri[[3, 40, 41]] = [-1, 9, 2 ** 31 - 1]
        check_kind(torch, rng, kind, rows, d, ids, dt, dt, row_index=ri)


# ---- B: geometry -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
def test_misaligned_views(torch, kind):
    """the table, the state or the gradient 1 element (V = 1) or 4 elements of a 16-bit type
    (8 bytes: V = 4) past a 16-byte boundary - one buffer at a time and all at once: the bits of
    the aligned call on the same data"""
    for dt, gdt in (("f32", "f32"), ("bf16", "bf16"), ("f16", "f32")):
        for d in (8, 64, 260):
            rng = np.random.default_rng(41 + d)
            ids = es.with_bad_ids(es.id_pattern(rng, "hubs", 50, 300), 50)
            data = (stored(rng, (50, d), dt), stored(rng, (300, d), gdt), make_state(rng, kind, (50, d)))
            aligned = check_kind(torch, rng, kind, 50, d, ids, dt, gdt, data=data)
            for shifts in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (4, 0, 0), (0, 0, 4), (4, 4, 4)):
                assert same_all(check_kind(torch, rng, kind, 50, d, ids, dt, gdt, shifts=shifts, data=data), aligned)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_the_same_call_gives_the_same_bits(torch, kind):
    rng = np.random.default_rng(61)
    table, state = stored(rng, (50, 64), "f32"), make_state(rng, kind, (50, 64))
    ids, grad = es.id_pattern(rng, "hubs", 50, 1000), es.sensitive_values(rng, (200, 64))
    a = run(torch, kind, table, "f32", state, ids, grad, "f32", count=5)
    b = run(torch, kind, table, "f32", state, ids, grad, "f32", count=5)
    assert same_all(a, b) and not es.same(a[0], table)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_one_long_segment(torch, kind):
    """1000 occurrences of a single id: 125 trips of the eight-ahead loop, and 1001 / 1003 for its
    tail; the order is kept - the bits are those of increasing positions, not of decreasing ones"""
    rng = np.random.default_rng(71)
    for e, d in ((1000, 4), (1001, 12), (1003, 1)):
        ids = np.full(e, 3, np.int64)
        data = (es.sensitive_values(rng, (7, d)), es.sensitive_values(rng, (e, d)), make_state(rng, kind, (7, d)))
        got = check_kind(torch, rng, kind, 7, d, ids, "f32", "f32", data=data)
        rev = ref.step(kind, data[0], "f32", data[2], ids, data[1], "f32", ref.scalars(kind, **HYPER), reverse=True)
        assert not same_all(got, rev)


def test_on_a_side_stream(torch):
    """one call inside torch.cuda.stream(...): ordered on that stream, the same bits"""
    from euler_amd import ops
    rng = np.random.default_rng(81)
    rows, d, count = 50, 64, 5
    table, grad, state = stored(rng, (rows, d), "bf16"), stored(rng, (200, d), "f32"), make_state(rng, "adam", (rows, d))
    ids = es.with_bad_ids(es.id_pattern(rng, "hubs", rows, 1000), rows)
    t, t_ids, t_grad = dev(torch, table, "bf16")[0], torch.from_numpy(ids).cuda(), torch.from_numpy(grad).cuda()
    st = [torch.from_numpy(s).cuda() for s in state]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.sparse_row_step("adam", t, t_ids, t_grad, st, step=2, count=count, **HYPER)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    want = ref.step("adam", table, "bf16", state, ids, grad, "f32", ref.scalars("adam", step=2, **HYPER), count=count)
    assert same_all((host(torch, t), [host(torch, s) for s in st]), want)


def test_windows_past_the_grid_cap(torch):
    """the launcher keeps the stores' cap of 8192 blocks of four waves, 64 sorted entries a
    wave-trip: with E = 8192 * 4 * 64 + 1000 = 2^21 + 1000 the last windows are a wave's second
    trip.  d = 1 and rows = 50; the gradient chain per id is np.cumsum over fp32 from the first occurrence - a
    sequential chain, as asserted on 1000 entries against the loop first - and the step on the
    summed rows is the restatement's on one occurrence per id"""
    from euler_amd import ops
    rng = np.random.default_rng(91)
    rows, e = 50, 8192 * 4 * 64 + 1000
    table, state = es.sensitive_values(rng, (rows, 1)), make_state(rng, "adam", (rows, 1))
    ids, grad = rng.integers(-1, rows + 1, e), es.sensitive_values(rng, (e, 1))
    sc = ref.scalars("adam", step=3, **HYPER)

    def summed(ids, grad):
        live = [i for i in range(rows) if np.any(ids == i)]
        g = np.stack([np.cumsum(grad[ids == i, 0], dtype=np.float32)[-1:] for i in live])
        return ref.step("adam", table, "f32", state, np.array(live, np.int64), g, "f32", sc)

    assert same_all(summed(ids[:1000], grad[:1000]), ref.step("adam", table, "f32", state, ids[:1000], grad[:1000], "f32", sc))
    t, guard = dev(torch, table, "f32", extra_rows=1)
    st = [torch.from_numpy(s).cuda() for s in state]
    ops.sparse_row_step("adam", t, torch.from_numpy(ids).cuda(), torch.from_numpy(grad).cuda(), st, step=3, **HYPER)
    assert same_all((host(torch, t), [host(torch, s) for s in st]), summed(ids, grad)) and guard_ok(torch, guard)


# ---- C: the optimiser classes ----------------------------------------------------------------
def _make_optimizer(name, params):
    from euler_amd import optim
    if name == "adam":
        return optim.SparseAdam(params, lr=HYPER["lr"], betas=HYPER["betas"], eps=1e-8), "adam"
    if name == "adagrad":
        return optim.SparseAdagrad(params, lr=HYPER["lr"], initial_accumulator_value=0.1, eps=1e-10), "adagrad"
    mu = 0.9 if name == "momentum" else 0.0
    return optim.SparseSGD(params, lr=HYPER["lr"], momentum=mu), name


def _initial_state(kind, shape):
    z = np.zeros(shape, np.float32)
    return {"sgd": [], "momentum": [z], "adagrad": [np.full(shape, 0.1, np.float32)], "adam": [z, z.copy()]}[kind]


STATE_KEYS = {"sgd": [], "momentum": ["momentum_buffer"], "adagrad": ["sum"], "adam": ["exp_avg", "exp_avg_sq"]}


@pytest.mark.parametrize("name", ["adam", "adagrad", "sgd", "momentum"])
@pytest.mark.parametrize("loss", ["skipgram", "triple"])
@pytest.mark.parametrize("dts", [("f32", "f32"), ("bf16", "f16")])
def test_optimizers_over_three_rounds(torch, name, loss, dts):
    """three backward() / step() rounds on tables of 50 rows, d = 12 (both fp32, or one bf16 and
    one fp16: the gradient is of the table's dtype and the state stays fp32), the gradients those
    of skipgram_loss / triple_score with sparse_grad=True: after every round each table and its
    state have the bits of the restatement called with the gradient's indices and values"""
    from euler_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(3)
    rows, d = 50, 12
    tables = [torch.nn.Parameter((torch.randn((rows, d), device="cuda", generator=gen) * 0.3).to(tdt(torch, dt)))
              for dt in dts]
    opt, kind = _make_optimizer(name, tables)
    want = [(host(torch, p), _initial_state(kind, (rows, d))) for p in tables]
    for t in (1, 2, 3):
        ids = lambda *shape: torch.randint(-1, rows + 1, shape, device="cuda", generator=gen)       # noqa: E731
        if loss == "skipgram":
            out, _ = ops.skipgram_loss(tables[0], tables[1], ids(40), ids(40, 2), ids(40, 5), sparse_grad=True)
        else:
            pos, neg = ops.triple_score(tables[0], tables[1], ids(40), ids(40), ids(40), ids(40, 5), sparse_grad=True)
            out = torch.relu(1.0 + neg.mean(1) - pos).mean() * 10
        opt.zero_grad()
        out.backward()
        opt.step()
        sc = ref.scalars(kind, step=t, **HYPER)
        for n, p in enumerate(tables):
            assert p.grad.is_sparse and p.grad._values().shape[0] > 0
            g_ids, g_rows = p.grad._indices()[0].cpu().numpy(), host(torch, p.grad._values())
            assert p.grad.dtype == p.dtype
            want[n] = ref.step(kind, want[n][0], dts[n], want[n][1], g_ids, g_rows, dts[n], sc)
            assert all(opt.state[p][k].dtype == torch.float32 for k in STATE_KEYS[kind])
            got = (host(torch, p), [host(torch, opt.state[p][k]) for k in STATE_KEYS[kind]])
            assert same_all(got, want[n]), (name, loss, t, n)
            if kind in ("adam", "adagrad"):
                assert opt.state[p]["step"] == t


@pytest.mark.parametrize("name", ["adam", "adagrad", "sgd", "momentum"])
def test_uncoalesced_and_coalesced_gradients(torch, name):
    """a hand-made sparse gradient with duplicate indices and its coalesce()d form: each matches
    the restatement for its own occurrence list (and the two lists differ)"""
    rng = np.random.default_rng(13)
    rows, d, e = 50, 12, 200
    table = es.sensitive_values(rng, (rows, d))
    ids, grad = es.id_pattern(rng, "hubs", rows, e), es.sensitive_values(rng, (e, d))
    g = torch.sparse_coo_tensor(torch.from_numpy(ids).reshape(1, -1).cuda(), torch.from_numpy(grad).cuda(), (rows, d))
    assert not g.is_coalesced()
    lists = []
    for sparse in (g, g.coalesce()):
        p = torch.nn.Parameter(torch.from_numpy(table).cuda())
        opt, kind = _make_optimizer(name, [p])
        p.grad = sparse
        opt.step()
        g_ids, g_rows = sparse._indices()[0].cpu().numpy(), host(torch, sparse._values())
        lists.append(len(g_ids))
        want = ref.step(kind, table, "f32", _initial_state(kind, (rows, d)), g_ids, g_rows, "f32", ref.scalars(kind, **HYPER))
        assert same_all((host(torch, p), [host(torch, opt.state[p][k]) for k in STATE_KEYS[kind]]), want)
        assert p.grad is sparse and sparse.is_coalesced() == (sparse is not g)        # the gradient is left as it came
    assert lists[0] == e and lists[1] < e


def test_checkpoints_round_trip_through_torch(torch):
    """state_dict() of optim.SparseAdam loads into torch.optim.SparseAdam and back: the keys and
    the step count are torch's, and the fused step continues from the loaded state bit for bit
    (an fp32 table: torch keeps state in the parameter's dtype, here the state's own)"""
    from euler_amd import optim
    rng = np.random.default_rng(19)
    rows, d = 50, 12
    table = es.sensitive_values(rng, (rows, d))

    def grad_of(seed):
        r = np.random.default_rng(seed)
        return torch.sparse_coo_tensor(torch.from_numpy(es.id_pattern(r, "hubs", rows, 100)).reshape(1, -1).cuda(),
                                       torch.from_numpy(es.sensitive_values(r, (100, d))).cuda(), (rows, d))

    p = torch.nn.Parameter(torch.from_numpy(table).cuda())
    a = optim.SparseAdam([p], lr=0.05)
    for seed in (1, 2):
        p.grad = grad_of(seed)
        a.step()
    sd = a.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and sd["state"][0]["step"] == 2
    q = torch.nn.Parameter(p.detach().clone())
    theirs = torch.optim.SparseAdam([q], lr=0.05)
    theirs.load_state_dict(copy.deepcopy(sd))          # (a copy, as a saved file is: load_state_dict keeps the tensors)
    assert theirs.state[q]["step"] == 2 and torch.equal(theirs.state[q]["exp_avg"], a.state[p]["exp_avg"])
    r = torch.nn.Parameter(p.detach().clone())
    back = optim.SparseAdam([r], lr=0.05)
    back.load_state_dict(copy.deepcopy(theirs.state_dict()))
    q.grad = grad_of(3)
    theirs.step()                                                          # torch's own step runs from it
    assert theirs.state[q]["step"] == 3
    for o, x in ((a, p), (back, r)):
        x.grad = grad_of(3)
        o.step()
    assert back.state[r]["step"] == 3 and es.same(host(torch, r), host(torch, p))
    assert all(es.same(host(torch, back.state[r][k]), host(torch, a.state[p][k])) for k in ("exp_avg", "exp_avg_sq"))


@pytest.mark.parametrize("name", ["adam", "adagrad", "momentum"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_checkpoints_of_16_bit_tables_resume(torch, name, dt):
    """a 16-bit table: the state is fp32, and stays fp32 with all its bits through state_dict()
    and load_state_dict() (torch's own load_state_dict would cast it to the table's dtype); the
    resumed optimiser steps on, bit for bit as the one that was never saved"""
    rng = np.random.default_rng(37)
    rows, d = 50, 12
    table = stored(rng, (rows, d), dt)

    def grad_of(seed):
        r = np.random.default_rng(seed)
        return torch.sparse_coo_tensor(torch.from_numpy(es.id_pattern(r, "hubs", rows, 100)).reshape(1, -1).cuda(),
                                       dev(torch, stored(r, (100, d), dt), dt)[0], (rows, d))

    p = torch.nn.Parameter(dev(torch, table, dt)[0])
    a, kind = _make_optimizer(name, [p])
    for seed in (1, 2):
        p.grad = grad_of(seed)
        a.step()
    sd = copy.deepcopy(a.state_dict())
    assert all(sd["state"][0][k].dtype == torch.float32 for k in STATE_KEYS[kind])
    q = torch.nn.Parameter(p.detach().clone())
    b, _ = _make_optimizer(name, [q])
    b.load_state_dict(sd)
    for k in STATE_KEYS[kind]:
        assert b.state[q][k].dtype == torch.float32 and b.state[q][k].device == q.device
        assert es.same(host(torch, b.state[q][k]), host(torch, a.state[p][k]))
        assert b.state[q][k].data_ptr() != sd["state"][0][k].data_ptr()
    assert int(b.state[q].get("step", 2)) == 2
    for o, x in ((a, p), (b, q)):
        x.grad = grad_of(3)
        o.step()
    assert es.same(host(torch, q), host(torch, p)) and not es.same(host(torch, p), table)
    assert all(es.same(host(torch, b.state[q][k]), host(torch, a.state[p][k])) for k in STATE_KEYS[kind])


# ---- D: refusals and version counters --------------------------------------------------------
def test_optimizer_refusals_and_empty_gradients(torch):
    from euler_amd import optim
    p = torch.nn.Parameter(torch.ones((7, 4), device="cuda"))
    q = torch.nn.Parameter(torch.ones((7, 4), device="cuda"))
    for make in (lambda ps: optim.SparseAdam(ps), lambda ps: optim.SparseAdagrad(ps, 0.1), lambda ps: optim.SparseSGD(ps, 0.1),
                 lambda ps: optim.get("momentum")(ps, 0.1)):
        opt = make([p, q])
        p.grad, q.grad = torch.ones((7, 4), device="cuda"), None
        with pytest.raises(RuntimeError, match="dense"):
            opt.step()
        p.grad = None
        q.grad = torch.sparse_coo_tensor(torch.tensor([[2, 2]], device="cuda"), torch.ones((2, 4), device="cuda"), (7, 4))
        before = q.detach().clone()
        opt.step()
        assert bool((p == 1).all()) and p not in opt.state                 # no gradient: untouched, no state
        moved = (q.detach() != before).any(1)
        assert moved.tolist() == [False, False, True, False, False, False, False]
        q.data.fill_(1.0)
    # an empty gradient still counts as a step, as torch.optim.SparseAdam counts it
    opt = optim.SparseAdam([p])
    p.grad = torch.sparse_coo_tensor(torch.zeros((1, 0), dtype=torch.int64, device="cuda"),
                                     torch.zeros((0, 4), device="cuda"), (7, 4))
    opt.step()
    opt.step()
    assert opt.state[p]["step"] == 2 and bool((p == 1).all()) and not bool(opt.state[p]["exp_avg"].any())
    with pytest.raises(ValueError):
        optim.SparseAdam([p], lr=-1.0)
    with pytest.raises(ValueError):
        optim.SparseAdam([p], betas=(1.0, 0.5))
    with pytest.raises(ValueError):
        optim.SparseSGD([p], 0.1, momentum=-0.5)


def test_python_refusals_and_version_counters(torch):
    from euler_amd import ops
    t = torch.zeros((7, 4), device="cuda", requires_grad=True)            # a leaf that requires grad: accepted
    ids = torch.tensor([1, 2, 2], device="cuda")
    g = torch.ones((3, 4), device="cuda")
    s0, s1 = torch.zeros((7, 4), device="cuda"), torch.zeros((7, 4), device="cuda")
    v = (t._version, s0._version, s1._version)
    assert ops.sparse_row_step("adam", t, ids, g, (s0, s1), lr=0.1) is t
    assert t._version > v[0] and s0._version > v[1] and s1._version > v[2]
    v = (t._version, s0._version)
    ops.sparse_row_step("momentum", t, ids, g, (s0,), lr=0.1, momentum=0.9)
    ops.sparse_row_step("adagrad", t, ids, g, (s1,), lr=0.1)
    assert t._version > v[0] + 1 and s0._version > v[1]
    v = t._version
    ops.sparse_row_step("sgd", t, ids, g, lr=0.1)
    assert t._version > v
    # a tensor autograd saved before the in-place call is detected as stale
    w = torch.ones((7, 4), device="cuda", requires_grad=True)
    y = (s0 * w).sum()
    ops.sparse_row_step("momentum", t, ids, g, (s0,), lr=0.1, momentum=0.9)
    with pytest.raises(RuntimeError):
        y.backward()
    snap = (t.detach().clone(), s0.clone(), s1.clone())
    bad = lambda *a, **k: ops.sparse_row_step(*a, **dict(dict(lr=0.1), **k))          # noqa: E731
    with pytest.raises(RuntimeError):
        bad("sgd", t * 1.0, ids, g)                                        # requires grad and is no leaf
    with pytest.raises(ValueError):
        bad("rmsprop", t, ids, g)
    with pytest.raises(ValueError):
        bad("sgd", torch.zeros((4, 7), device="cuda").t(), ids, g)         # table not contiguous
    with pytest.raises(ValueError):
        bad("momentum", t, ids, g, (torch.zeros((4, 7), device="cuda").t(),))        # state not contiguous
    with pytest.raises(ValueError):
        bad("momentum", t, ids, g, (torch.zeros((7, 5), device="cuda"),))  # state of the wrong shape
    with pytest.raises(ValueError):
        bad("momentum", t, ids, g, (torch.zeros((7, 4), device="cuda", dtype=torch.float16),))
    with pytest.raises(ValueError):
        bad("momentum", t, ids, g, (t.detach(),))                          # state shares storage with the table
    with pytest.raises(ValueError):
        bad("momentum", t, torch.arange(7, device="cuda"), s0, (s0,))      # ... with grad
    with pytest.raises(ValueError):
        bad("adam", t, ids, g, (s0, s0))                                   # ... with the other state tensor
    with pytest.raises(ValueError):
        bad("adam", t, ids, g, (s0,))                                      # one state tensor short
    with pytest.raises(ValueError):
        bad("sgd", t, ids, g, (s0,))
    with pytest.raises(ValueError):
        bad("sgd", t, ids, g.half())                                       # neither fp32 nor the table's dtype
    with pytest.raises(ValueError):
        bad("sgd", t, ids, g[:2])
    with pytest.raises(ValueError):
        bad("sgd", t, ids, g, row_index=torch.zeros(3, dtype=torch.int32, device="cuda"), count=3)
    with pytest.raises(ValueError):
        bad("sgd", t, ids.float(), g)
    with pytest.raises(ValueError):
        bad("sgd", t, ids, g, lr=-0.1)
    with pytest.raises(ValueError):
        bad("sgd", t, ids, g, lr=float("nan"))
    with pytest.raises(ValueError):
        bad("adam", t, ids, g, (s0, s1), step=0)
    with pytest.raises(ValueError):
        ops.sparse_row_step("sgd", t, ids, g)                              # no lr
    with pytest.raises(RuntimeError):
        bad("sgd", t.detach().cpu(), ids, g)
    assert bad("sgd", t, ids[:0], g[:0]) is t
    assert bad("adam", t, ids, g[:0], (s0, s1), row_index=torch.zeros(3, dtype=torch.int32, device="cuda")) is t
    assert all(torch.equal(a, b) for a, b in zip(snap, (t.detach(), s0, s1)))


def test_c_entry_refusals_leave_everything_untouched(torch):
    from euler_amd import _lib
    from euler_amd.ops import _stream
    L = _lib.lib()
    rows, d, e = 7, 8, 10
    table = torch.full((rows, d), 3.0, device="cuda")
    s0, s1 = torch.full((rows, d), 0.5, device="cuda"), torch.full((rows, d), 0.25, device="cuda")
    ids = torch.arange(e, device="cuda") % rows
    grad = torch.ones((e, d), device="cuda")
    ri = torch.zeros(e, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                                # noqa: E731
    base = dict(kind=3, table=p(table), dt=_lib.F32, rows=rows, d=d, s0=p(s0), s1=p(s1), ids=p(ids), e=e, grad=p(grad),
                gdt=_lib.F32, m=e, ri=None, count=0, lr=0.1, mu=0.0, eps=1e-8, om1=0.1, om2=0.001, step_size=0.1)

    def call(**kw):
        a = dict(base, **kw)
        rc = L.euler_gpu_sparse_optim_step(_stream(), a["kind"], a["table"], a["dt"], a["rows"], a["d"], a["s0"], a["s1"],
                                           a["ids"], a["e"], a["grad"], a["gdt"], a["m"], a["ri"], a["count"], a["lr"],
                                           a["mu"], a["eps"], a["om1"], a["om2"], a["step_size"])
        torch.cuda.synchronize()
        return rc

    EINVAL, OK = _lib.EINVAL, _lib.OK
    assert call(kind=4) == EINVAL and call(kind=-1) == EINVAL
    assert call(dt=3) == EINVAL and call(gdt=-1) == EINVAL
    assert call(gdt=_lib.BF16) == EINVAL and call(dt=_lib.F16, gdt=_lib.BF16) == EINVAL
    assert call(rows=0) == EINVAL
    assert call(e=1 << 31) == EINVAL and call(d=1 << 31) == EINVAL and call(e=-1) == EINVAL
    assert call(ri=p(ri), count=2, m=5) == EINVAL                          # both given
    assert call(count=-1) == EINVAL
    assert call(count=3, m=3) == EINVAL and call(count=2, m=4) == EINVAL   # e % count, m != e / count
    assert call(m=e - 1) == EINVAL
    assert call(table=None) == EINVAL and call(ids=None) == EINVAL and call(grad=None) == EINVAL
    assert call(s0=None) == EINVAL and call(s1=None) == EINVAL             # adam needs both
    assert call(kind=1) == EINVAL and call(kind=2) == EINVAL               # momentum / adagrad: one, not two
    assert call(kind=1, s0=None, s1=None) == EINVAL and call(kind=0) == EINVAL and call(kind=0, s1=None) == EINVAL
    assert call(table=C.c_void_p(table.data_ptr() + 2)) == EINVAL
    assert call(grad=C.c_void_p(grad.data_ptr() + 1)) == EINVAL
    assert call(ids=C.c_void_p(ids.data_ptr() + 4)) == EINVAL
    assert call(ri=C.c_void_p(ri.data_ptr() + 2)) == EINVAL
    assert call(s0=C.c_void_p(s0.data_ptr() + 2)) == EINVAL and call(s1=C.c_void_p(s1.data_ptr() + 1)) == EINVAL
    for name in ("lr", "mu", "eps", "om1", "om2", "step_size"):
        assert call(**{name: -0.5}) == EINVAL and call(**{name: float("nan")}) == EINVAL
        assert call(**{name: float("inf")}) == EINVAL
    assert call(e=0, m=0) == OK and call(d=0) == OK and call(e=0, m=0, table=None, ids=None, grad=None) == OK
    assert call(ri=p(ri), m=0, grad=None) == OK                            # no source row: every occurrence is removed
    assert bool((table == 3.0).all()) and bool((s0 == 0.5).all()) and bool((s1 == 0.25).all())
    # and the full call still works afterwards, for every kind
    assert call() == OK and call(kind=2, s1=None) == OK and call(kind=1, s1=None) == OK
    assert call(kind=0, s0=None, s1=None) == OK
    assert not bool((table == 3.0).any()) and not bool((s0 == 0.5).any()) and not bool((s1 == 0.25).any())


# ---- E: the examples -------------------------------------------------------------------------
@pytest.mark.parametrize("script,args", [
    ("deepwalk_train.py", ["--nodes", "2000", "--batch", "16", "--steps", "1", "--dim", "32"]),
    ("transe_minibatch.py", []),
    ("transh_transd_minibatch.py", []),
    ("transr_minibatch.py", []),
    ("shallow_encoder_minibatch.py", []),
])
def test_examples_with_the_fused_optimizer(script, args):
    """one step of each example with --fused-optimizer: the example itself asserts that only rows
    its gradient names moved, and reports how many did"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", script), "--fused-optimizer"] + args,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("fused optimizer:")]
    assert len(line) == 1 and "all of them looked up" in line[0] and int(line[0].split()[2]) > 0, r.stdout
