"""The in-place embedding stores on the GPU (ops.embedding_update / embedding_add / embedding_take,
euler_gpu_store_update / _add / _take).  Every comparison is bit equality against the sequential
numpy restatement tests/embed_store_ref.py:
  A  bits over d x E x rows, the id patterns, ids that name no row, a guard row behind the table
  B  dtypes (table x values / out), special values, the count and row_index forms, misaligned views
  C  the order of add is observable and kept; take reads the table as it was; repeatability
  D  the Python checks, the version counter, the rules of the C entries, a side stream
  E  a window past the launcher's grid cap (the grid-stride trip)
  F  the example's step and its fused-against-composed check"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
import embed_store_ref as ref

pytestmark = pytest.mark.gpu

DIMS = [1, 3, 4, 8, 12, 64, 130, 260]
SIZES = [0, 1, 63, 64, 65, 1000]
ROWS = [1, 7, 50]


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
        guard.view(torch.int16 if dt != "f32" else torch.int32).fill_(0x7bcd)
    return view, guard


def host(torch, t):
    """a cuda tensor -> its numpy storage (float32, or uint16 bits)"""
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def guard_ok(torch, guard):
    return bool((guard.view(torch.int16 if guard.dtype != torch.float32 else torch.int32) == 0x7bcd).all())


def stored(rng, shape, dt):
    return ref.narrow(ref.sensitive_values(rng, shape), dt)


def check_all(torch, rng, rows, d, ids, dt, vdt, row_index=None, count=None, shift=0, tag=()):
    """update, add, take, take + clear on the device == the restatement, the guard row included"""
    from euler_amd import ops
    e = len(ids)
    m = e // count if count else (9 if row_index is not None else e)
    table, values = stored(rng, (rows, d), dt), stored(rng, (m, d), vdt)
    t_ids = torch.from_numpy(ids).cuda()
    t_values, _ = dev(torch, values, vdt, shift)
    t_ri = None if row_index is None else torch.from_numpy(row_index).cuda()
    tag = tag + (rows, d, e, dt, vdt, count, row_index is not None, shift)
    for name, fn, want in (("update", ops.embedding_update, ref.update), ("add", ops.embedding_add, ref.add)):
        t, guard = dev(torch, table, dt, shift, extra_rows=1)
        back = fn(t, t_ids, t_values, row_index=t_ri, count=count)
        assert back is t
        assert ref.same(host(torch, t), want(table, dt, ids, values, vdt, row_index, count)), (name,) + tag
        assert guard_ok(torch, guard), (name, "guard") + tag
    for clear in (False, True):
        t, guard = dev(torch, table, dt, shift, extra_rows=1)
        out = ops.embedding_take(t, t_ids, clear=clear, out_dtype=tdt(torch, vdt))
        want_out, want_after = ref.take(table, dt, ids, clear, vdt)
        assert out.shape == (e, d) and out.dtype == tdt(torch, vdt)
        assert ref.same(host(torch, out), want_out) and ref.same(host(torch, t), want_after), ("take", clear) + tag
        assert guard_ok(torch, guard), ("take", clear, "guard") + tag


# ---- A: bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_bits_of_the_restatement(torch, d):
    """every E x rows; the id pattern, ids that name no row (-1, rows, 2^40, -2^63), the table's
    dtype and the values' dtype rotate through the cases"""
    rng = np.random.default_rng(100 + d)
    n = DIMS.index(d)
    for e in SIZES:
        for rows in ROWS:
            ids = ref.id_pattern(rng, ref.PATTERNS[n % len(ref.PATTERNS)], rows, e)
            if n % 2:
                ids = ref.with_bad_ids(ids, rows)
            dt = ref.DTYPES[n % 3]
            check_all(torch, rng, rows, d, ids, dt, dt if (n // 3) % 2 else "f32")
            n += 1


@pytest.mark.parametrize("pattern", ref.PATTERNS)
def test_id_patterns(torch, pattern):
    """all distinct (rows 2000 >= E), all equal, two hubs, sorted, reverse sorted, random - with
    and without ids that name no row"""
    rng = np.random.default_rng(11)
    for d in (4, 130):
        rows = 2000 if pattern == "distinct" else 50
        ids = ref.id_pattern(rng, pattern, rows, 1000 if pattern != "equal" else 300)
        if pattern == "distinct":
            assert len(np.unique(ids)) == len(ids)
        check_all(torch, rng, rows, d, ids, "f32", "f32", tag=(pattern,))
        check_all(torch, rng, rows, d, ref.with_bad_ids(ids, rows), "bf16", "f32", tag=(pattern, "bad"))


# ---- B: dtypes and forms ---------------------------------------------------------------------
@pytest.mark.parametrize("dt", ref.DTYPES)
@pytest.mark.parametrize("other", ["f32", "same"])
def test_dtypes(torch, dt, other):
    """table fp32 / bf16 / fp16 x values (and out) fp32 / the table's dtype; out_dtype=None is the
    table's dtype"""
    from euler_amd import ops
    rng = np.random.default_rng(21)
    vdt = "f32" if other == "f32" else dt
    for d in (3, 8, 12):
        rows = 50
        ids = ref.with_bad_ids(ref.id_pattern(rng, "hubs", rows, 1000), rows, every=9)
        check_all(torch, rng, rows, d, ids, dt, vdt)
    t, _ = dev(torch, stored(rng, (7, 8), dt), dt)
    out = ops.embedding_take(t, torch.tensor([[1, 2], [3, -1]], device="cuda"))
    assert out.dtype == tdt(torch, dt) and out.shape == (2, 2, 8)
    assert ref.same(host(torch, out).reshape(4, 8), ref.take(host(torch, t), dt, [1, 2, 3, -1])[0])


@pytest.mark.parametrize("dt", ref.DTYPES)
def test_same_dtype_update_copies_bits(torch, dt):
    """-0.0 and a NaN payload arrive bit for bit; take returns them bit for bit"""
    from euler_amd import ops
    neg0, nan = {"f32": (0x80000000, 0x7fc12345), "bf16": (0x8000, 0x7fc5), "f16": (0x8000, 0x7e05)}[dt]
    view = np.uint32 if dt == "f32" else np.uint16
    store = np.float32 if dt == "f32" else np.uint16
    for d in (3, 8):
        table = np.full((7, d), nan, view).view(store)
        values = np.array([[neg0, nan, 1] + [neg0] * (d - 3)] * 3, view).view(store)
        ids = np.array([2, -1, 5], np.int64)
        t, guard = dev(torch, table, dt, extra_rows=1)
        ops.embedding_update(t, torch.from_numpy(ids).cuda(), dev(torch, values, dt)[0])
        got = host(torch, t)
        assert ref.same(got, ref.update(table, dt, ids, values, dt)) and guard_ok(torch, guard)
        assert got.view(view)[2].tolist() == values.view(view)[0].tolist()
        assert np.all(got.view(view)[[0, 1, 3, 4, 6]] == nan)
        out = ops.embedding_take(t, torch.from_numpy(ids).cuda())
        assert ref.same(host(torch, out), ref.take(got, dt, ids)[0])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_count_and_row_index_forms(torch, dt):
    """both forms == the plain call on the materialised block (equal bits); a row_index entry
    outside [0, M) removes its occurrence; both given is an error"""
    from euler_amd import ops
    rng = np.random.default_rng(31)
    rows, count = 50, 5
    for d in (12, 64):
        ids = ref.with_bad_ids(ref.id_pattern(rng, "hubs", rows, 200 * count), rows, every=11)
        check_all(torch, rng, rows, d, ids, dt, "f32", count=count)
        ri = rng.integers(0, 9, len(ids)).astype(np.int32)
        ri[[3, 40, 41]] = [-1, 9, 2 ** 31 - 1]
        check_all(torch, rng, rows, d, ids, dt, dt, row_index=ri)
        # against the materialised form on the device
        table, v9, v200 = stored(rng, (rows, d), dt), stored(rng, (9, d), "f32"), stored(rng, (200, d), "f32")
        t_ids = torch.from_numpy(ids).cuda()
        for fn in (ops.embedding_update, ops.embedding_add):
            block, keep = ref.materialise(v9, 9, row_index=ri)
            a, b = dev(torch, table, dt)[0], dev(torch, table, dt)[0]
            fn(a, t_ids, dev(torch, v9, "f32")[0], row_index=torch.from_numpy(ri).cuda())
            fn(b, torch.from_numpy(np.where(keep, ids, -1)).cuda(), dev(torch, block, "f32")[0])
            assert torch.equal(a.view(torch.int16 if dt != "f32" else torch.int32),
                               b.view(torch.int16 if dt != "f32" else torch.int32))
            block, keep = ref.materialise(v200, 200, count=count)
            a, b = dev(torch, table, dt)[0], dev(torch, table, dt)[0]
            fn(a, t_ids, dev(torch, v200, "f32")[0], count=count)
            fn(b, t_ids, dev(torch, block, "f32")[0])
            assert keep.all() and ref.same(host(torch, a), host(torch, b))
    t = dev(torch, stored(rng, (rows, 4), dt), dt)[0]
    with pytest.raises(ValueError):
        ops.embedding_add(t, torch.zeros(10, dtype=torch.int64, device="cuda"), torch.zeros((2, 4), device="cuda"),
                          row_index=torch.zeros(10, dtype=torch.int32, device="cuda"), count=5)


@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_misaligned_views(torch, dt):
    """table, values and out one element past a 16-byte boundary (V = 1): the bits of the aligned call"""
    rng = np.random.default_rng(41)
    for d in (8, 64, 260):
        ids = ref.with_bad_ids(ref.id_pattern(rng, "hubs", 50, 1000), 50)
        check_all(torch, np.random.default_rng(5), 50, d, ids, dt, "f32", shift=1)
        check_all(torch, np.random.default_rng(5), 50, d, ids, dt, "f32", shift=0)      # the same data, aligned
        check_all(torch, rng, 50, d, ids, dt, dt, count=5, shift=1)
        # out one element past a 16-byte boundary: through the C entry (ops allocates its own out)
        from euler_amd import _lib
        from euler_amd.ops import _stream
        table = stored(rng, (50, d), dt)
        t, t_ids = dev(torch, table, dt)[0], torch.from_numpy(ids).cuda()
        for odt in (dt, "f32"):
            out, guard = dev(torch, ref.zeros((len(ids), d), odt), odt, shift=1, extra_rows=1)
            rc = _lib.lib().euler_gpu_store_take(_stream(), C.c_void_p(t.data_ptr()), ref.DTYPES.index(dt), 50,
                                                 d, C.c_void_p(t_ids.data_ptr()), len(ids), 0,
                                                 C.c_void_p(out.data_ptr()), ref.DTYPES.index(odt))
            torch.cuda.synchronize()
            assert rc == 0 and ref.same(host(torch, out), ref.take(table, dt, ids, False, odt)[0]) and guard_ok(torch, guard)


# ---- C: order, take, repeatability -----------------------------------------------------------
def test_order_of_add_is_observable_and_kept(torch):
    """first on the restatement: 300 occurrences of one id added in reversed position order change
    bits in every column, and the first and last duplicate carry different rows; then the device
    has the bits of the forward order, and update keeps the last duplicate"""
    from euler_amd import ops
    rng = np.random.default_rng(5)
    table = np.zeros((7, 4), np.float32)
    ids = ref.id_pattern(rng, "equal", 7, 300)
    values = ref.sensitive_values(rng, (300, 4))
    fwd, rev = ref.add(table, "f32", ids, values, "f32"), ref.add(table, "f32", ids, values, "f32", reverse=True)
    assert np.all(fwd[3].view(np.uint32) != rev[3].view(np.uint32))
    assert not ref.same(values[0], values[-1])
    t_ids, t_values = torch.from_numpy(ids).cuda(), torch.from_numpy(values).cuda()
    t = torch.from_numpy(table).cuda()
    ops.embedding_add(t, t_ids, t_values)
    assert ref.same(host(torch, t), fwd) and not ref.same(host(torch, t), rev)
    ops.embedding_update(t, t_ids, t_values)
    assert ref.same(host(torch, t)[3], values[-1])


def test_take_reads_the_table_as_it_was(torch):
    """duplicates all return the old row; clear=True leaves the named rows at +0 and the others
    untouched; clear=False leaves the table bit-identical"""
    from euler_amd import ops
    rng = np.random.default_rng(51)
    for d in (3, 64, 260):
        table = stored(rng, (50, d), "f32")
        ids = ref.with_bad_ids(ref.id_pattern(rng, "hubs", 50, 1000), 50, every=7)
        ids[ids == 13] = 14                                               # row 13 is named by no id
        t_ids = torch.from_numpy(ids).cuda()
        t = torch.from_numpy(table).cuda()
        out = ops.embedding_take(t, t_ids)
        assert ref.same(host(torch, t), table)
        named = (ids >= 0) & (ids < 50)
        assert ref.same(host(torch, out)[named], table[ids[named]]) and not host(torch, out)[~named].any()
        out2 = ops.embedding_take(t, t_ids, clear=True)
        assert ref.same(host(torch, out2), host(torch, out))
        after = host(torch, t)
        touched = np.zeros(50, bool)
        touched[ids[named]] = True
        assert not touched[13] and ref.same(after[~touched], table[~touched])
        assert ref.same(after[touched], np.zeros((int(touched.sum()), d), np.float32))


def test_the_same_call_gives_the_same_bits(torch):
    from euler_amd import ops
    rng = np.random.default_rng(61)
    table = torch.from_numpy(stored(rng, (50, 64), "f32")).cuda()
    ids = torch.from_numpy(ref.id_pattern(rng, "hubs", 50, 1000)).cuda()
    values = torch.from_numpy(ref.sensitive_values(rng, (200, 64))).cuda()
    a, b = table.clone(), table.clone()
    ops.embedding_add(a, ids, values, count=5)
    ops.embedding_add(b, ids, values, count=5)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.equal(a, table)


# ---- D: the Python checks and the C entries --------------------------------------------------
def test_version_counter_and_python_checks(torch):
    from euler_amd import ops
    t = torch.zeros((7, 4), device="cuda")
    ids = torch.tensor([1, 2, 2], device="cuda")
    v = torch.ones((3, 4), device="cuda")
    v0 = t._version
    assert ops.embedding_update(t, ids, v) is t and t._version > v0
    v1 = t._version
    assert ops.embedding_add(t, ids, v) is t and t._version > v1
    v2 = t._version
    ops.embedding_take(t, ids)
    assert t._version == v2
    ops.embedding_take(t, ids, clear=True)
    assert t._version > v2
    # a tensor autograd saved before the in-place call is detected as stale
    w = torch.ones((7, 4), device="cuda", requires_grad=True)
    y = (t * w).sum()
    ops.embedding_add(t, ids, v)
    with pytest.raises(RuntimeError):
        y.backward()
    for fn in (lambda x: ops.embedding_update(x, ids, v), lambda x: ops.embedding_add(x, ids, v),
               lambda x: ops.embedding_take(x, ids)):
        with pytest.raises(RuntimeError):
            fn(torch.zeros((7, 4), device="cuda", requires_grad=True))
    with pytest.raises(ValueError):
        ops.embedding_update(t.double(), ids, v.double())
    with pytest.raises(ValueError):
        ops.embedding_update(t, ids, v.half())                          # neither fp32 nor the table's dtype
    with pytest.raises(ValueError):
        ops.embedding_update(t, ids, v[:2])
    with pytest.raises(ValueError):
        ops.embedding_update(t, ids, torch.ones((3, 5), device="cuda"))
    with pytest.raises(ValueError):
        ops.embedding_add(t, ids, v[:2], count=2)
    with pytest.raises(ValueError):
        ops.embedding_add(t, ids, v, row_index=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.embedding_take(t.t(), ids)                                  # not contiguous
    with pytest.raises(ValueError):
        ops.embedding_take(t, ids.float())
    with pytest.raises(RuntimeError):
        ops.embedding_take(t.cpu(), ids)
    assert ops.embedding_take(t, ids[:0]).shape == (0, 4) and ops.embedding_take(t[:, :0], ids).shape == (3, 0)
    assert ops.embedding_add(t, ids[:0], v[:0]) is t


def test_c_entry_error_rules_leave_the_table_untouched(torch):
    from euler_amd import _lib
    from euler_amd.ops import _stream
    L = _lib.lib()
    rows, d, e = 7, 8, 10
    table = torch.full((rows, d), 3.0, device="cuda")
    ids = torch.arange(e, device="cuda") % rows
    values = torch.ones((e, d), device="cuda")
    out = torch.full((e, d), -5.0, device="cuda")
    ri = torch.zeros(e, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                                # noqa: E731
    base = dict(table=p(table), dt=_lib.F32, rows=rows, d=d, ids=p(ids), e=e, values=p(values), vdt=_lib.F32, m=e,
                ri=None, count=0, clear=1, out=p(out), odt=_lib.F32)

    def write(fn, **kw):
        a = dict(base, **kw)
        rc = fn(_stream(), a["table"], a["dt"], a["rows"], a["d"], a["ids"], a["e"], a["values"], a["vdt"], a["m"],
                a["ri"], a["count"])
        torch.cuda.synchronize()
        return rc

    def take(**kw):
        a = dict(base, **kw)
        rc = L.euler_gpu_store_take(_stream(), a["table"], a["dt"], a["rows"], a["d"], a["ids"], a["e"], a["clear"],
                                    a["out"], a["odt"])
        torch.cuda.synchronize()
        return rc

    EINVAL, OK = _lib.EINVAL, _lib.OK
    for fn in (L.euler_gpu_store_update, L.euler_gpu_store_add):
        w = lambda **kw: write(fn, **kw)                                  # noqa: E731
        assert w(dt=3) == EINVAL and w(vdt=-1) == EINVAL
        assert w(vdt=_lib.BF16) == EINVAL and w(dt=_lib.F16, vdt=_lib.BF16) == EINVAL
        assert w(rows=0) == EINVAL
        assert w(e=1 << 31) == EINVAL and w(d=1 << 31) == EINVAL
        assert w(ri=p(ri), count=2, m=5) == EINVAL                        # both given
        assert w(count=-1) == EINVAL
        assert w(count=3, m=3) == EINVAL and w(count=2, m=4) == EINVAL    # e % count, m != e / count
        assert w(m=e - 1) == EINVAL
        assert w(table=None) == EINVAL and w(ids=None) == EINVAL and w(values=None) == EINVAL
        assert w(table=C.c_void_p(table.data_ptr() + 2)) == EINVAL
        assert w(values=C.c_void_p(values.data_ptr() + 1)) == EINVAL
        assert w(ids=C.c_void_p(ids.data_ptr() + 4)) == EINVAL
        assert w(ri=C.c_void_p(ri.data_ptr() + 2)) == EINVAL
        assert w(e=0, m=0) == OK and w(d=0) == OK and w(e=0, m=0, table=None, ids=None, values=None) == OK
    assert take(dt=3) == EINVAL and take(odt=_lib.BF16) == EINVAL and take(rows=0) == EINVAL
    assert take(e=1 << 31) == EINVAL and take(d=1 << 31) == EINVAL
    assert take(table=None) == EINVAL and take(ids=None) == EINVAL and take(out=None) == EINVAL
    assert take(out=C.c_void_p(out.data_ptr() + 2)) == EINVAL
    assert take(e=0) == OK and take(d=0) == OK
    assert bool((table == 3.0).all()) and bool((out == -5.0).all())
    # and the full calls still work afterwards
    assert write(L.euler_gpu_store_add) == OK and take() == OK
    assert out[:, 0].tolist() == [5.0] * 3 + [4.0] * 4 + [5.0] * 3 and not bool(table.any())


def test_on_a_side_stream(torch):
    """the three ops inside torch.cuda.stream(...): ordered on that stream, the same bits"""
    from euler_amd import ops
    rng = np.random.default_rng(71)
    rows, d, count = 50, 64, 5
    table, values = stored(rng, (rows, d), "bf16"), stored(rng, (200, d), "f32")
    ids = ref.with_bad_ids(ref.id_pattern(rng, "hubs", rows, 1000), rows)
    t, t_ids, t_values = dev(torch, table, "bf16")[0], torch.from_numpy(ids).cuda(), torch.from_numpy(values).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.embedding_update(t, t_ids, t_values, count=count)
        ops.embedding_add(t, t_ids, t_values, count=count)
        out = ops.embedding_take(t, t_ids, clear=True, out_dtype=torch.float32)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    want = ref.add(ref.update(table, "bf16", ids, values, "f32", count=count), "bf16", ids, values, "f32", count=count)
    want_out, want_after = ref.take(want, "bf16", ids, True, "f32")
    assert ref.same(host(torch, out), want_out) and ref.same(host(torch, t), want_after)


# ---- E: past the grid cap --------------------------------------------------------------------
def test_windows_past_the_grid_cap(torch):
    """the launcher caps the grid at 8192 blocks of four waves, 64 sorted entries a wave-trip: with
    E = 2^21 * 4 + 1000 the last windows are a wave's second trip.  d = 1 and rows = 50; the
    restatement per id is np.cumsum over fp32 - a sequential chain, as asserted on 1000 entries
    against the loop first"""
    from euler_amd import ops
    rng = np.random.default_rng(81)
    rows, e = 50, 8192 * 4 * 64 + 1000

    def chain(table, ids, values):
        out = table.copy()
        for i in range(rows):
            v = values[ids == i, 0]
            if len(v):
                out[i, 0] = np.cumsum(np.concatenate([table[i], v]), dtype=np.float32)[-1]
        return out

    table = ref.sensitive_values(rng, (rows, 1))
    ids, values = rng.integers(-1, rows + 1, e), ref.sensitive_values(rng, (e, 1))
    assert ref.same(chain(table, ids[:1000], values[:1000]), ref.add(table, "f32", ids[:1000], values[:1000], "f32"))
    t, guard = dev(torch, table, "f32", extra_rows=1)
    t_ids, t_values = torch.from_numpy(ids).cuda(), torch.from_numpy(values).cuda()
    ops.embedding_add(t, t_ids, t_values)
    added = chain(table, ids, values)
    assert ref.same(host(torch, t), added)
    out = ops.embedding_take(t, t_ids, clear=True)
    named = (ids >= 0) & (ids < rows)
    want = np.where(named, added[np.clip(ids, 0, rows - 1), 0], np.float32(0)).astype(np.float32).reshape(e, 1)
    assert ref.same(host(torch, out), want) and not host(torch, t).any()
    ops.embedding_update(t, t_ids, t_values)
    last = np.zeros((rows, 1), np.float32)
    for i in range(rows):
        last[i] = values[np.nonzero(ids == i)[0][-1]]
    assert ref.same(host(torch, t), last) and guard_ok(torch, guard)


# ---- F: the example --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example():
    spec = importlib.util.spec_from_file_location(
        "scalable_sage_minibatch", os.path.join(ROOT, "examples", "python", "scalable_sage_minibatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("store", ["fp32", "bf16"])
def test_example_step_on_a_synthetic_graph(torch, example, store):
    """step() on a 2 000-node synthetic graph, fused and composed: finite losses, the stores move
    only in rows the batch names, the row past the table stays +0; and on distinct ids the fused
    and the composed store operations agree (update and take exactly, add within its bound)"""
    import euler_amd
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[store]
    nodes, batch, fanout, dim = 2000, 64, 10, 32
    for composed in (False, True):
        G = euler_amd.Graph.synthetic(euler_amd.synth_params(1, nodes, 10 * nodes, weighted=True))
        G.set_seed(42)
        feat = torch.randn((nodes + 2, 16), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        s = example.State(G, nodes, feat, 16, dim, 8, fanout, dt)
        before = s.store_buf.clone()
        inputs = torch.arange(1, batch + 1, device="cuda")
        loss, neighbor = example.step(s, inputs, composed)
        assert bool(torch.isfinite(loss))
        moved = (s.store_buf != before).any(1)
        assert bool(moved[inputs].all()) and int(moved.sum()) == batch and not bool(s.store_buf[-1].any())
        # the gradient store holds what the neighbours that are not in the batch were handed
        held = s.grad_buf.float().abs().sum(1) > 0
        in_batch = torch.zeros(nodes + 2, dtype=torch.bool, device="cuda")
        in_batch[inputs] = True
        assert not bool(held[in_batch].any()) and not bool(held[-1])
        live = neighbor[(neighbor >= 0) & (neighbor <= nodes)]
        outside = torch.zeros(nodes + 2, dtype=torch.bool, device="cuda")
        outside[live] = True
        assert not bool(held[~outside].any())
        loss2, _ = example.step(s, inputs, composed)
        assert bool(torch.isfinite(loss2))
    worst = example.compare(s.store, s.grad_store, batch, fanout)
    print("\n[scalable_sage %s] fused against composed add: worst |diff| / bound = %.4f" % (store, worst))
    assert 0 <= worst <= 1
