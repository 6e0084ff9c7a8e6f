"""Every one of the sixteen segment-reduce entries called once through the C ABI, against the numpy
restatements (mp_base_ref / weighted_mp_ref), bit for bit: what a swapped or dropped field in an
entry's adapter (MpReduceCall, mp_segments.h) would change.

Shapes: a 7-row table, 5 destinations, 15 updates (count 3).  d = 12 takes the element kernels
(fp32: 12 / 4 = 3 lanes do not divide 64; 16-bit: 12 % 8 != 0), d = 16 the 16-byte-lane kernels
(with 2 heads dh = 8, so the weighted vector form stays eligible for fp32 and 16-bit rows).
seg_ptr is ragged with an empty destination; the scatter keys are unsorted (the sort path) and
one equals `size` (left out); of the int64 ids one lies past the table and one is -1 (both read
the last row).  16-bit storage S: out fp32 has the bits of the fp32 op on the widened
input, out S those bits after one rounding - the equality test_weighted_mp_gpu.py asks for."""
import ctypes as C

import numpy as np
import pytest

import mp_base_ref as base
import weighted_mp_ref as wref
from test_mp_entry_args_host import ARGS

pytestmark = pytest.mark.gpu

ROWS, SIZE, E, COUNT = 7, 5, 15, 3
OPS = ["add", "max", "mean"]
SEG_PTR = np.array([0, 4, 4, 9, 10, 15], np.int64)                   # destination 1 is empty
KEYS = np.array([3, 0, 4, 1, 5, 2, 0, 3, 3, 1, 4, 0, 2, 4, 1], np.int32)      # unsorted; 5 == size
F32, BF16, F16 = 0, 1, 2


@pytest.fixture(scope="module", params=[12, 16])
def case(request, torch_cuda):
    """inputs on the device and the fp32 references of every form, computed once per d"""
    torch = torch_cuda
    d = request.param
    rng = np.random.default_rng(100 + d)
    # multiples of 1/8 in [-4, 4): exact in bf16 and fp16, so every storage type holds the same values
    draw = lambda *shape: (rng.integers(-32, 32, shape) / 8.0).astype(np.float32)
    x, upd = draw(ROWS, d), draw(E, d)
    gi = rng.integers(0, ROWS, E).astype(np.int32)
    ids = gi.astype(np.int64)
    ids[2], ids[7], ids[11] = ROWS + 3, -1, (1 << 33) + 2            # past the table; -1; only the low word counts
    id_rows = base.id_rows(ids, ROWS)
    w = {h: draw(E, h) for h in (1, 2)}
    by_count, by_ptr = base.segment_keys(SIZE, count=COUNT), base.segment_keys(SIZE, seg_ptr=SEG_PTR)
    want = {}
    for op in OPS:
        want["scatter", op] = base.scatter_ref(op, upd, KEYS, SIZE)
        want["gather_scatter", op] = base.gather_scatter_ref(op, x, gi, KEYS, SIZE)
        want["segment", "count", op] = base.gather_scatter_ref(op, x, gi, by_count, SIZE)
        want["segment", "ptr", op] = base.gather_scatter_ref(op, x, gi, by_ptr, SIZE)
        want["segment_ids", "count", op] = base.gather_scatter_ref(op, x, id_rows, by_count, SIZE)
        want["segment_ids", "ptr", op] = base.gather_scatter_ref(op, x, id_rows, by_ptr, SIZE)
        for h in (1, 2):
            want["gather_scatter_w", op, h] = wref.gather_scatter_ref(op, x, gi, KEYS, SIZE, w[h])
            want["segment_w", "count", op, h] = wref.gather_scatter_ref(op, x, gi, by_count, SIZE, w[h])
            want["segment_w", "ptr", op, h] = wref.gather_scatter_ref(op, x, gi, by_ptr, SIZE, w[h])
            want["segment_ids_w", "count", op, h] = wref.gather_scatter_ref(op, x, id_rows, by_count, SIZE, w[h])
            want["segment_ids_w", "ptr", op, h] = wref.gather_scatter_ref(op, x, id_rows, by_ptr, SIZE, w[h])
    dev = lambda a: torch.from_numpy(a).cuda()
    return dict(d=d, x=dev(x), upd=dev(upd), gi=dev(gi), ids=dev(ids), keys=dev(KEYS), seg_ptr=dev(SEG_PTR),
                w={h: dev(w[h]) for h in w}, want={k: dev(v) for k, v in want.items()})


def _call(torch, entry, out_type, **a):
    """one raw call with the arguments of ARGS[entry] taken from a (tensors as pointers) -> out"""
    from euler_amd import _lib
    out = torch.full((SIZE, a["d"]), 77.0, dtype=out_type, device="cuda")
    a = dict(a, out=out, size=SIZE)
    values = [C.c_void_p(v.data_ptr()) if isinstance(v, torch.Tensor) else v for v in (a[n] for n in ARGS[entry])]
    rc = getattr(_lib.lib(), "euler_gpu_" + entry)(None, *values)
    assert rc == 0, (entry, _lib.lib().euler_gpu_last_error().decode())
    return out


def _same(torch, got, want):
    return got.dtype == want.dtype and torch.equal(got.view(torch.int32 if got.dtype == torch.float32 else torch.int16),
                                                   want.view(torch.int32 if want.dtype == torch.float32 else torch.int16))


def _check_typed(torch, fp32_entry, want, fixed, data, weights=None):
    """the fp32 entry (mode first unless it has none), its `_t` twin with fp32 codes - the same
    bits - and the twin over bf16 / fp16 storage; data: the name of the argument that holds the rows"""
    typed = "scatter_t" if fp32_entry.startswith("scatter_") else fp32_entry + "_t"
    got = _call(torch, fp32_entry, torch.float32, **fixed, **({} if weights is None else {"w": weights}))
    assert _same(torch, got, want), fp32_entry
    wd = {} if weights is None else {"w": weights, "w_dtype": F32}
    twin = _call(torch, typed, torch.float32, in_dtype=F32, out_dtype=F32, **fixed, **wd)
    assert _same(torch, twin, got), typed + " fp32"
    for code, S in ((BF16, torch.bfloat16), (F16, torch.float16)):
        rows = dict(fixed, **{data: fixed[data].to(S)})
        for wS in ([None] if weights is None else [(F32, weights), (code, weights.to(S))]):
            wd = {} if wS is None else {"w": wS[1], "w_dtype": wS[0]}
            got32 = _call(torch, typed, torch.float32, in_dtype=code, out_dtype=F32, **rows, **wd)
            assert _same(torch, got32, want), (typed, S, "out fp32")
            gotS = _call(torch, typed, S, in_dtype=code, out_dtype=code, **rows, **wd)
            assert _same(torch, gotS, want.to(S)), (typed, S, "out S")


@pytest.mark.parametrize("op", OPS)
def test_scatter_entries(torch_cuda, case, op):
    c = case
    fixed = dict(mode=OPS.index(op), params=c["upd"], keys=c["keys"], e=E, d=c["d"])
    _check_typed(torch_cuda, "scatter_" + op, c["want"]["scatter", op], fixed, "params")


@pytest.mark.parametrize("op", OPS)
def test_gather_scatter_entries(torch_cuda, case, op):
    c = case
    fixed = dict(mode=OPS.index(op), params=c["x"], gather=c["gi"], keys=c["keys"], e=E, d=c["d"])
    _check_typed(torch_cuda, "gather_scatter", c["want"]["gather_scatter", op], fixed, "params")
    for h in (1, 2):
        _check_typed(torch_cuda, "gather_scatter_w", c["want"]["gather_scatter_w", op, h], dict(fixed, heads=h),
                     "params", c["w"][h])


@pytest.mark.parametrize("form", ["count", "ptr"])
@pytest.mark.parametrize("op", OPS)
def test_segment_entries(torch_cuda, case, op, form):
    c = case
    seg = dict(seg_ptr=None, count=COUNT) if form == "count" else dict(seg_ptr=c["seg_ptr"], count=0)
    fixed = dict(seg, mode=OPS.index(op), params=c["x"], d=c["d"], params_rows=ROWS)
    for entry, gather in (("segment", c["gi"]), ("segment_ids", c["ids"])):
        name = "gather_segment_reduce" + entry[len("segment"):]
        _check_typed(torch_cuda, name, c["want"][entry, form, op], dict(fixed, gather=gather), "params")
        for h in (1, 2):
            _check_typed(torch_cuda, name + "_w", c["want"][entry + "_w", form, op, h],
                         dict(fixed, gather=gather, heads=h), "params", c["w"][h])
