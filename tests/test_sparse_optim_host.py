"""The shared pieces of the fused sparse-row optimiser steps (euler_amd/csrc/sparse_optim.h),
compiled with the host compiler alone and driven over whole calls, against the numpy restatement
tests/sparse_optim_ref.py: bit equality of sgd / momentum / adagrad / adam.  Also: state carried
over three steps, the order of the gradient chain, the fp32 result within the running bound of the
float64 twin, the twin against torch's own optimisers in float64, untouched rows, and the entry's
export and binding.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import embed_store_ref as es
import sparse_optim_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
CODE = {"f32": 0, "bf16": 1, "f16": 2}
DIMS = [1, 3, 4, 8, 12, 64, 130, 260]
SIZES = [0, 1, 63, 64, 65, 1000]
ROWS = [1, 7, 50]
HYPER = dict(lr=0.05, momentum=0.9, betas=(0.9, 0.999))


@pytest.fixture(scope="module")
def SO():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libsparse_optim_check.so")
    src = os.path.join(HERE, "csrc", "sparse_optim_check.cc")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", h)
                    for h in ("sparse_optim.h", "embed_store.h", "mp_weighted.h", "half_cvt.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # the host compiler alone, no HIP header; -ffp-contract=off as the library's build
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    L.so_call.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64] + [C.c_float] * 6
    L.so_call.restype = C.c_int
    L.so_chunk_width.argtypes = [C.c_int64, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64]
    L.so_state_count.argtypes = [C.c_int32]
    return L


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def host(L, kind, table, dt, state, ids, grad, gdt, sc, row_index=None, count=0):
    """one call of the host build on COPIES -> (the table, the list of state arrays) afterwards"""
    t = np.array(table, copy=True)
    st = [np.array(s, dtype=np.float32, copy=True) for s in state] + [None, None]
    ids = np.ascontiguousarray(ids, np.int64)
    grad = np.ascontiguousarray(grad)
    ri = None if row_index is None else np.ascontiguousarray(row_index, np.int32)
    rc = L.so_call(ref.KINDS.index(kind), ptr(t), CODE[dt], t.shape[0], t.shape[1], ptr(st[0]), ptr(st[1]), ptr(ids),
                   len(ids), ptr(grad), CODE[gdt], grad.shape[0], ptr(ri), count or 0,
                   sc["lr"], sc["mu"], sc["eps"], sc["om1"], sc["om2"], sc["step_size"])
    assert rc == 0
    return t, st[:len(state)]


def stored(rng, shape, dt):
    """order-sensitive values stored as dt"""
    return es.narrow(es.sensitive_values(rng, shape), dt)


def make_state(rng, kind, shape):
    """fp32 state of a kind: the accumulators of squares (adagrad's sum, adam's exp_avg_sq) are
    positive, the others signed"""
    v = es.sensitive_values(rng, shape)
    return {"sgd": [], "momentum": [v], "adagrad": [np.abs(v)],
            "adam": [v, np.abs(es.sensitive_values(rng, shape))]}[kind]


def same_all(got, want):
    return es.same(got[0], want[0]) and len(got[1]) == len(want[1]) and all(es.same(a, b) for a, b in zip(got[1], want[1]))


def check_kind(L, rng, kind, rows, d, ids, dt, gdt, row_index=None, count=0, step=1):
    e = len(ids)
    m = e // count if count else (9 if row_index is not None else e)
    table, grad, state = stored(rng, (rows, d), dt), stored(rng, (m, d), gdt), make_state(rng, kind, (rows, d))
    sc = ref.scalars(kind, step=step, **HYPER)
    got = host(L, kind, table, dt, state, ids, grad, gdt, sc, row_index, count)
    want = ref.step(kind, table, dt, state, ids, grad, gdt, sc, row_index, count or None)
    assert same_all(got, want), (kind, rows, d, e, dt, gdt, count, row_index is not None)


@pytest.mark.parametrize("d", DIMS)
def test_host_build_equals_the_restatement(SO, d):
    """every E x rows x kind; the id patterns, ids that name no row, the table's dtype and the
    gradient's dtype (fp32 / the table's) rotate so that every kind meets every dtype pair"""
    rng = np.random.default_rng(200 + d)
    n = 0
    for e in SIZES:
        for rows in ROWS:
            for kind in ref.KINDS:
                pattern, bad = ref.rotation(n)
                ids = es.id_pattern(rng, es.PATTERNS[pattern], rows, e)
                if bad:
                    ids = es.with_bad_ids(ids, rows)
                dt = es.DTYPES[n % 3]
                check_kind(SO, rng, kind, rows, d, ids, dt, dt if (n // 12) % 2 else "f32", step=1 + n % 5)
                n += 1


def test_the_rotation_meets_every_combination():
    """kind x table dtype x gradient dtype, and id pattern x ids that name no row"""
    cases = range(len(SIZES) * len(ROWS) * 4)
    assert len({(n % 4, n % 3, (n // 12) % 2) for n in cases}) == 4 * 3 * 2
    assert {ref.rotation(n) for n in cases} == {(p, bad) for p in range(len(es.PATTERNS)) for bad in (False, True)}


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("dt", es.DTYPES)
def test_count_and_row_index_forms(SO, kind, dt):
    """the count and row_index forms == the restatement, and the restatement of a form == the
    plain form on the materialised block; a row_index entry outside [0, M) removes its occurrence"""
    rng = np.random.default_rng(7)
    rows, d, count = 50, 12, 5
    ids = es.with_bad_ids(es.id_pattern(rng, "hubs", rows, 60 * count), rows, every=11)
    check_kind(SO, rng, kind, rows, d, ids, dt, "f32", count=count)
    ri = rng.integers(0, 9, len(ids)).astype(np.int32)
    ri[[3, 40, 41]] = [-1, 9, 2 ** 31 - 1]
    check_kind(SO, rng, kind, rows, d, ids, dt, dt, row_index=ri)
    sc = ref.scalars(kind, **HYPER)
    table, state = stored(rng, (rows, d), dt), make_state(rng, kind, (rows, d))
    g9, g60 = stored(rng, (9, d), dt), stored(rng, (60, d), dt)
    block, keep = es.materialise(g9, 9, row_index=ri)
    assert not keep[3] and not keep[40] and not keep[41]
    assert same_all(ref.step(kind, table, dt, state, ids, g9, dt, sc, row_index=ri),
                    ref.step(kind, table, dt, state, np.where(keep, ids, -1), block, dt, sc))
    block, keep = es.materialise(g60, 60, count=count)
    assert keep.all()
    assert same_all(ref.step(kind, table, dt, state, ids, g60, dt, sc, count=count),
                    ref.step(kind, table, dt, state, ids, block, dt, sc))


@pytest.mark.parametrize("kind", ref.KINDS)
def test_three_steps_with_the_state_carried(SO, kind):
    """the table and the state of one step feed the next; adam's step_size changes with t"""
    rng = np.random.default_rng(17)
    for dt, gdt in (("f32", "f32"), ("bf16", "f32"), ("f16", "f16")):
        rows, d = 50, 12
        a = b = (stored(rng, (rows, d), dt), make_state(rng, kind, (rows, d)))
        sizes = set()
        for t in (1, 2, 3):
            sc = ref.scalars(kind, step=t, **HYPER)
            sizes.add(sc["step_size"])
            ids = es.with_bad_ids(es.id_pattern(rng, "hubs", rows, 300), rows, every=13)
            grad = stored(rng, (300, d), gdt)
            a = host(SO, kind, a[0], dt, a[1], ids, grad, gdt, sc)
            b = ref.step(kind, b[0], dt, b[1], ids, grad, gdt, sc)
            assert same_all(a, b), (kind, dt, t)
        assert len(sizes) == 3


@pytest.mark.parametrize("kind", ref.KINDS)
def test_the_order_of_the_gradient_chain(SO, kind):
    """300 occurrences of one id: the restatement summed in decreasing position differs in bits in
    every buffer that is linear in g - every state buffer, and the table of sgd and momentum
    (adagrad and adam step by about lr * sign(g) here, which the last bits of g need not move);
    the host build has the bits of the increasing order"""
    rng = np.random.default_rng(5)
    table, state = es.sensitive_values(rng, (7, 4)), make_state(rng, kind, (7, 4))
    ids = es.id_pattern(rng, "equal", 7, 300)
    grad = es.sensitive_values(rng, (300, 4))
    sc = ref.scalars(kind, **HYPER)
    fwd = ref.step(kind, table, "f32", state, ids, grad, "f32", sc)
    rev = ref.step(kind, table, "f32", state, ids, grad, "f32", sc, reverse=True)
    linear = ([fwd[0]] if kind in ("sgd", "momentum") else []) + fwd[1]
    other = ([rev[0]] if kind in ("sgd", "momentum") else []) + rev[1]
    for a, b in zip(linear, other):
        assert np.any(a[3].view(np.uint32) != b[3].view(np.uint32))
    got = host(SO, kind, table, "f32", state, ids, grad, "f32", sc)
    assert same_all(got, fwd) and not same_all(got, rev)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_fp32_within_the_running_bound_of_float64(SO, kind, capsys):
    """three steps, the state and its bound carried: |fp32 - twin| <= the twin's running bound, per
    element of the table and of every state buffer, no margin (the derivation: sparse_optim_ref)"""
    worst = 0.0
    for seed, (rows, e, name) in enumerate(((7, 300, "equal"), (50, 1000, "hubs"), (50, 1000, "random"), (7, 65, "sorted"))):
        rng = np.random.default_rng(40 + seed)
        d = 12
        a = (es.sensitive_values(rng, (rows, d)), make_state(rng, kind, (rows, d)))
        b, bounds = a, None
        for t in (1, 2, 3):
            sc = ref.scalars(kind, step=t, **HYPER)
            ids = es.with_bad_ids(es.id_pattern(rng, name, rows, e), rows, every=13)
            grad = es.sensitive_values(rng, (e, d))
            a = host(SO, kind, a[0], "f32", a[1], ids, grad, "f32", sc)
            b, bounds = ref.step64(kind, b[0], b[1], ids, grad, sc, bounds=bounds)
            for got, want, bound in zip([a[0]] + a[1], [b[0]] + b[1], [bounds[0]] + bounds[1]):
                err = np.abs(got.astype(np.float64) - want)
                assert np.all(err <= bound), (kind, name, t, float((err / np.maximum(bound, 1e-300)).max()))
                worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    with capsys.disabled():
        print("\n[sparse_row_step %s] worst error / bound = %.4f" % (kind, worst))
    assert 0 < worst <= 1


def _torch_optimizer(torch, kind, p):
    if kind == "adam":
        return torch.optim.SparseAdam([p], lr=HYPER["lr"], betas=HYPER["betas"], eps=1e-8)
    if kind == "adagrad":
        return torch.optim.Adagrad([p], lr=HYPER["lr"], initial_accumulator_value=0.1, eps=1e-10)
    return torch.optim.SGD([p], lr=HYPER["lr"], momentum=0)


@pytest.mark.parametrize("kind", ["sgd", "adagrad", "adam"])
def test_the_twin_against_torch_in_float64(kind, capsys):
    """torch.optim.SGD (momentum 0), Adagrad (initial_accumulator_value) and SparseAdam on CPU
    float64 tensors, the gradient an UNCOALESCED sparse tensor, three steps, against the twin with
    double scalars.  The bound is the twin's derivation with u = 2^-53 in its free form, B per
    element, times the factor that sparse_optim_ref's docstring derives per kind and per row:
    2 for adam and adagrad (twin to exact + torch to exact), and N + 2 for a row of sgd, N the
    most occurrences that row had in a step so far (torch may fold them into the row one by one).
    momentum has no torch counterpart with touched-rows-only semantics (torch.optim.SGD refuses
    momentum with sparse gradients): it is checked against the twin alone, above."""
    import torch
    rng = np.random.default_rng(23)
    rows, d, e = 50, 12, 300
    table = es.sensitive_values(rng, (rows, d)).astype(np.float64)
    p = torch.tensor(table, requires_grad=True)
    opt = _torch_optimizer(torch, kind, p)
    state = {"sgd": [], "adagrad": [np.full((rows, d), 0.1)], "adam": [np.zeros((rows, d)), np.zeros((rows, d))]}[kind]
    b, bounds, most, worst = (table, state), None, np.zeros(rows, np.int64), 0.0
    for t in (1, 2, 3):
        ids = es.id_pattern(rng, ("hubs", "random", "equal")[t - 1], rows, e)
        grad = es.sensitive_values(rng, (e, d)).astype(np.float64)
        p.grad = torch.sparse_coo_tensor(torch.from_numpy(ids).reshape(1, -1), torch.from_numpy(grad), (rows, d))
        assert not p.grad.is_coalesced()
        opt.step()
        sc = ref.scalars(kind, step=t, fp32=False, **HYPER)
        b, bounds = ref.step64(kind, b[0], b[1], ids, grad, sc, u=ref.U64, bounds=bounds, free=True)
        most = np.maximum(most, ref.occurrence_counts(ids, rows, e))
        factor = ref.torch_factor(kind, most)[:, None]
        tstate = {"sgd": [], "adagrad": ["sum"], "adam": ["exp_avg", "exp_avg_sq"]}[kind]
        got = [p.detach().numpy()] + [opt.state[p][k].numpy() for k in tstate]
        for g, want, bound in zip(got, [b[0]] + b[1], [bounds[0]] + bounds[1]):
            err, allowed = np.abs(g - want), factor * bound
            ratio = float((err[allowed > 0] / allowed[allowed > 0]).max())
            assert np.all(err <= allowed), (kind, t, "worst error / (factor * B) = %.4f" % ratio)
            worst = max(worst, ratio)
        moved = most > 0
        assert 0 < moved.sum() and es.same(got[0][~moved].astype(np.float32), table[~moved].astype(np.float32))
    with capsys.disabled():
        print("\n[twin against torch, %s] worst error / (factor * B) = %.4f" % (kind, worst))
    assert 0 <= worst <= 1 and most.min() < 5 and most.max() == e


@pytest.mark.parametrize("kind", ref.KINDS)
def test_untouched_rows_keep_their_bits(SO, kind):
    """rows no live id names hold a NaN-payload sentinel in the table and the state: it survives"""
    rng = np.random.default_rng(29)
    for dt, nan in (("f32", 0x7fc12345), ("bf16", 0x7fc5), ("f16", 0x7e05)):
        rows, d = 50, 12
        ids = es.with_bad_ids(es.id_pattern(rng, "hubs", rows, 200), rows, every=7)
        ids[ids == 13] = 14
        ri = rng.integers(0, 9, len(ids)).astype(np.int32)
        dead = np.nonzero(ids == 20)[0]
        ri[dead] = -1                                                     # row 20: named, but by no LIVE occurrence
        live = np.zeros(rows, bool)
        live[[int(i) for i in ref.occurrences(ids, rows, 9, ri)]] = True
        assert not live[13] and not live[20] and live.sum() > 10
        table, state = stored(rng, (rows, d), dt), make_state(rng, kind, (rows, d))
        view = np.uint32 if dt == "f32" else np.uint16
        table.view(view)[~live] = nan
        for s in state:
            s.view(np.uint32)[~live] = 0x7fc12345
        grad = stored(rng, (9, d), dt)
        sc = ref.scalars(kind, **HYPER)
        got = host(SO, kind, table, dt, state, ids, grad, dt, sc, row_index=ri)
        assert same_all(got, ref.step(kind, table, dt, state, ids, grad, dt, sc, row_index=ri))
        assert np.all(got[0].view(view)[~live] == nan) and not np.any(got[0].view(view)[live] == nan)
        for s in got[1]:
            assert np.all(s.view(np.uint32)[~live] == 0x7fc12345) and not np.any(s.view(np.uint32)[live] == 0x7fc12345)


def test_chunk_width_counts_the_state(SO):
    assert [SO.so_state_count(k) for k in range(4)] == [0, 1, 1, 2]
    assert SO.so_chunk_width(64, 32, 4, 64, 4, 0, 0) == 8 and SO.so_chunk_width(64, 32, 4, 64, 4, 96, 128) == 8
    assert SO.so_chunk_width(64, 32, 4, 64, 4, 100, 128) == 1 and SO.so_chunk_width(64, 32, 4, 64, 4, 96, 132) == 1
    assert SO.so_chunk_width(12, 32, 4, 64, 4, 96, 0) == 4 and SO.so_chunk_width(64, 8, 2, 16, 2, 96, 0) == 4
    assert SO.so_chunk_width(64, 32, 4, 68, 4, 96, 128) == 1 and SO.so_chunk_width(130, 32, 4, 64, 4, 96, 0) == 1


def test_the_entry_is_exported_and_bound():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    name = "euler_gpu_sparse_optim_step"
    assert name in _lib.SIGNATURES and hasattr(L, name) and name + "(" in hdr
    assert len(_lib.SIGNATURES[name][1]) == 21 and _lib.SIGNATURES[name][1][-6:] == [C.c_float] * 6
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.parametrize("dt", ["bfloat16", "float16", "float32"])
def test_load_state_dict_keeps_the_state_fp32(dt):
    """the state of a 16-bit table is fp32; torch's load_state_dict would cast it to the table's
    dtype - the classes' own keeps every bit, on the parameter's device, in tensors of its own
    (no step runs here: loading needs no GPU)"""
    import torch
    from euler_amd import optim
    rng = np.random.default_rng(31)
    p = torch.nn.Parameter(torch.zeros((7, 4), dtype=getattr(torch, dt)))
    for make, keys in ((lambda: optim.SparseAdam([p], lr=0.05), ("exp_avg", "exp_avg_sq")),
                       (lambda: optim.SparseAdagrad([p], lr=0.05), ("sum",)),
                       (lambda: optim.SparseSGD([p], lr=0.05, momentum=0.9), ("momentum_buffer",))):
        saved = {k: torch.from_numpy(es.sensitive_values(rng, (7, 4))) for k in keys}
        sd = make().state_dict()
        sd["state"] = {0: dict(saved, step=5)}
        opt = make()
        opt.load_state_dict(sd)
        assert opt.state[p]["step"] == 5
        for k in keys:
            got = opt.state[p][k]
            assert got.dtype == torch.float32 and got.device == p.device and got.data_ptr() != saved[k].data_ptr()
            assert es.same(got.numpy(), saved[k].numpy())
            assert not torch.equal(saved[k].to(p.dtype).float(), saved[k]) or dt == "float32"
        again = opt.state_dict()
        assert all(es.same(again["state"][0][k].numpy(), saved[k].numpy()) for k in keys)


def test_the_python_surface_is_public():
    from euler_amd import ops, optim
    assert callable(ops.sparse_row_step)
    assert all(callable(optim.get(n)) for n in ("sgd", "momentum", "adagrad", "adam"))
    assert optim.get("adagrad") is optim.SparseAdagrad and optim.get("adam") is optim.SparseAdam
    assert optim.get("rmsprop") is None                                  # dict.get, as the reference's
