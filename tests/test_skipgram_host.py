"""The per-lane arithmetic of the fused skip-gram loss head (euler_amd/csrc/skipgram.h), compiled
with the host compiler, against the numpy restatement tests/skipgram_ref.py: bit equality of the
logits, the row and total loss, the rank and the three gradient blocks; the corner cases of the
softplus and of the sigmoid; the tie rule of the rank against the reference's double argsort; the
measured ulp constants; the restatement within the derived bound of the float64 formulation.
CPU only.  Also: the new C-ABI entries are exported and bound."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import skipgram_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
f32p, i64p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
F = np.float32
LN2 = F(0.6931472)                                               # fl(ln 2)
L1P_WORST_BITS, SP_WORST_BITS = 0x3b7d1600, 0xc03072d0           # where E_L1P / E_SP occur (skipgram_ref.py)


@pytest.fixture(scope="module")
def SG():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libskipgram_check.so")
    src = os.path.join(HERE, "csrc", "skipgram_check.cc")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", h)
                    for h in ("skipgram.h", "kg_score.h", "mp_softmax.h", "mp_weighted.h", "sparse_embed.h", "half_cvt.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # the host compiler alone, no HIP header; -ffp-contract=off as the library's build
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    L.sg_chunk_width.argtypes = [C.c_int64, f32p, f32p]
    L.sg_chunk_width.restype = C.c_int
    for name in ("sg_log1p", "sg_sigmoid"):
        getattr(L, name).argtypes = [f32p, C.c_int64, f32p]
        getattr(L, name).restype = None
    L.sg_term.argtypes = [f32p, C.c_int64, C.c_int32, f32p]
    L.sg_term.restype = None
    L.sg_coef.argtypes = [C.c_float, f32p, C.c_int64, C.c_int32, f32p]
    L.sg_coef.restype = None
    L.sg_total.argtypes = [f32p, C.c_int64, C.c_int64, C.c_int64]
    L.sg_total.restype = C.c_float
    L.sg_log1p_error.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.sg_log1p_error.restype = C.c_double
    L.sg_softplus_error.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    L.sg_softplus_error.restype = C.c_double
    L.sg_pairs.argtypes = [C.c_int32, f32p, C.c_int64, f32p, C.c_int64, i64p, i64p, i64p] + [C.c_int64] * 4 + \
        [f32p, i32p, f32p, f32p, f32p, C.c_float, f32p, f32p, f32p]
    L.sg_pairs.restype = C.c_int
    return L


def placed(a, shift=0):
    """a copy of fp32 `a` whose first element lies `shift` elements past a 16-byte boundary"""
    buf = np.empty(a.size + 8, np.float32)
    at = (-(buf.ctypes.data // 4)) % 4 + shift
    out = buf[at:at + a.size].reshape(a.shape)
    out[...] = a
    assert out.ctypes.data % 16 == 4 * shift % 16
    return out


def fp(a):
    return a.ctypes.data_as(f32p) if a is not None else None


def ip(a):
    return a.ctypes.data_as(i64p) if a is not None else None


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


def unary(fn, x, *extra, lead=()):
    """fn(*lead, x, n, *extra, out) -> out"""
    x = np.ascontiguousarray(x, F)
    out = np.full_like(x, np.nan)
    fn(*lead, fp(x), x.size, *extra, fp(out))
    return out


def run(L, target, context, src, pos, neg, v=0, logits=None, g=0.0):
    """the host build: forward -> (logits, rank, row_loss, loss); with logits the gradient -> the three blocks"""
    b, d, p = len(src), target.shape[1], pos.shape[1]
    k = 0 if neg is None else neg.shape[1]
    src, pos = np.ascontiguousarray(src, np.int64), np.ascontiguousarray(pos, np.int64)
    neg = None if neg is None else np.ascontiguousarray(neg, np.int64)
    head = (v, fp(target), target.shape[0], fp(context), context.shape[0], ip(src), ip(pos), ip(neg), b, p, k, d)
    if logits is None:
        out, rank = np.full((b, p + k), np.nan, F), np.full(b, -7, np.int32)
        row_loss, loss = np.full(b, np.nan, F), np.full(1, np.nan, F)
        assert L.sg_pairs(*head, fp(out), rank.ctypes.data_as(i32p), fp(row_loss), fp(loss), None, 0.0,
                          None, None, None) == 0
        return out, rank, row_loss, loss[0]
    gs, gp, gn = np.full((b, d), np.nan, F), np.full((b, p, d), np.nan, F), np.full((b, k, d), np.nan, F)
    assert L.sg_pairs(*head, None, None, None, None, fp(np.ascontiguousarray(logits, F)), g, fp(gs), fp(gp), fp(gn)) == 0
    return gs, gp, gn


def tables(rng, d, rows_t=40, rows_c=37, shift=0, scale=True):
    def one(rows):
        x = rng.random((rows, d)) * 2 - 1
        if scale:
            x = x * 10.0 ** rng.integers(-2, 2, (rows, d))
        return placed(x.astype(F), shift)
    return one(rows_t), one(rows_c)


def batch(rng, b, p, k, rows_t, rows_c):
    return rng.integers(0, rows_t, b), rng.integers(0, rows_c, (b, p)), (rng.integers(0, rows_c, (b, k)) if k else None)


def check_both(L, target, context, src, pos, neg, rng, v=0):
    """forward and gradient bits of the host build == the restatement; -> (forward, gradient)"""
    d = target.shape[1]
    vv = v or ref.chunk_width(d, target.ctypes.data, 4, context.ctypes.data, 4)
    assert v or vv == L.sg_chunk_width(d, fp(target), fp(context))
    tag = (d, vv, len(src), pos.shape[1], 0 if neg is None else neg.shape[1])
    got = run(L, target, context, src, pos, neg, v)
    want = ref.forward(target, context, src, pos, neg, vv)
    assert same(got[0], want[0]), tag + ("logits",)
    assert got[1].dtype == want[1].dtype == np.int32 and np.array_equal(got[1], want[1]), tag + ("rank",)
    assert same(got[2], want[2]), tag + ("row_loss",)
    assert same(F(got[3]), F(want[3])), tag + ("loss",)
    g = float(F(rng.random() * 4 - 2))
    got_g = run(L, target, context, src, pos, neg, v, logits=got[0], g=g)
    want_g = ref.grad(target, context, src, pos, neg, want[0], g)
    for a, w, name in zip(got_g, want_g, ("src", "pos", "neg")):
        assert same(a, w), tag + (name,)
    return got, got_g


@pytest.mark.parametrize("d", ref.DIMS)
def test_host_build_equals_the_restatement(SG, d):
    """V = 1 / 4 / 8 by d, one and several chunks a lane, every butterfly width; P in {1, 2} x
    K in {0, 1, 5} x B in {1, 90}; B = 300 and 513 cross the 256 partials of the total"""
    rng = np.random.default_rng(100 + d)
    target, context = tables(rng, d)
    for p in (1, 2):
        for k in (0, 1, 5):
            for b in (1, 90):
                check_both(SG, target, context, *batch(rng, b, p, k, 40, 37), rng)
    for b in (255, 256, 257, 300, 513):
        check_both(SG, target, context, *batch(rng, b, 1, 5, 40, 37), rng)


@pytest.mark.parametrize("d", [8, 64, 520])
def test_unaligned_table_start_and_forced_widths(SG, d):
    """tables one element past a 16-byte boundary take V = 1; V forced to 1, 4 and 8"""
    rng = np.random.default_rng(7 + d)
    target, context = tables(rng, d, shift=1)
    assert ref.chunk_width(d, target.ctypes.data, 4, context.ctypes.data, 4) == 1 == \
        SG.sg_chunk_width(d, fp(target), fp(context))
    src, pos, neg = batch(rng, 9, 2, 5, 40, 37)
    check_both(SG, target, context, src, pos, neg, rng)
    for v in (1, 4, 8):
        check_both(SG, target, context, src, pos, neg, rng, v=v)
    # the same table as target and as context (LINE's first order)
    check_both(SG, target, target, src, np.minimum(pos, 39), neg, rng)


def test_total_order_is_a_function_of_b(SG):
    """sg_total == the restatement for B around every partial boundary; an empty input gives +0"""
    rng = np.random.default_rng(5)
    for b in (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000):
        rl = (rng.random(b) * 10.0 ** rng.integers(-3, 3, b)).astype(F)
        got = F(SG.sg_total(fp(rl) if b else None, b, 2, 5))
        assert same(got, F(ref.total(rl, b, 2, 5))), b
    assert F(SG.sg_total(None, 0, 1, 0)).view(np.uint32) == 0


def test_log1p_and_softplus_fixed_points(SG):
    """Log1pUnit at e = 0, 1 and the smallest normal e; the terms at logits 0, +-86, +-1e4"""
    tiny = F(2.0 ** -126)
    e = np.array([0.0, 1.0, tiny], F)
    got = unary(SG.sg_log1p, e)
    assert same(got, ref.log1p_unit(e))
    assert got[0].view(np.uint32) == 0 and got[1] == LN2 and got[2] == tiny
    x = np.array([0.0, -0.0, 86.0, -86.0, 1e4, -1e4, 86.5, -86.5], F)
    for positive in (True, False):
        got = unary(SG.sg_term, x, int(positive))
        assert same(got, ref.term(x, positive))
        assert got[0] == LN2 and got[1] == LN2                           # max(+-0, 0) is +0
        big = got[2:].reshape(3, 2)                                      # (x, -x) pairs
        shrinks, grows = (big[:, 0], big[:, 1]) if positive else (big[:, 1], big[:, 0])
        # softplus of the large side is the logit itself (86 + 4.5e-38 rounds to 86), of the other
        # side exp(-86) > 0 at 86 and exactly +0 beyond the floor
        assert np.array_equal(grows, np.array([86.0, 1e4, 86.5], F))
        assert shrinks[0] > 0 and shrinks[0] < 1e-37 and shrinks[1].view(np.uint32) == 0 and shrinks[2].view(np.uint32) == 0
        assert not np.any(np.signbit(got))


def test_sigmoid_is_exact_where_e_is_zero(SG):
    x = np.array([0.0, 86.0, -86.0, 86.5, -86.5, 1e4, -1e4, 3.0, -3.0], F)
    sig = unary(SG.sg_sigmoid, x)
    assert same(sig, ref.sigmoid(x))
    assert sig[0] == 0.5 and sig[3] == 1 and sig[5] == 1 and sig[4].view(np.uint32) == 0 and sig[6].view(np.uint32) == 0
    assert 0 < sig[2] < 1e-37 and sig[1] == 1                            # (1 / (1 + 4.5e-38) rounds to 1)
    assert same(sig[7:], np.array([F(1) / (F(1) + ref.exp_of(F(3))), ref.exp_of(F(3)) / (F(1) + ref.exp_of(F(3)))], F))
    gs = F(0.37)
    for positive in (True, False):
        c = unary(SG.sg_coef, x, int(positive), lead=(gs,))
        assert same(c, ref.coef(gs, x, positive))
    cp, cn = unary(SG.sg_coef, x, 1, lead=(gs,)), unary(SG.sg_coef, x, 0, lead=(gs,))
    # e = 0: a positive at +1e4 passes exactly 0, at -1e4 exactly -gs; a negative gs and 0
    assert cp[5] == 0 and cp[6] == -gs and cn[5] == gs and cn[6] == 0 and cp[3] == 0 and cn[4] == 0


def test_measured_ulp_constants_are_not_exceeded(SG):
    """E_L1P and E_SP were measured over every fp32 argument; here the same measure
    on a stride through the bit patterns plus windows around every power of two, the ends and the
    recorded worst arguments, held against the constants"""
    worst = C.c_uint32(0)
    one = int(np.array(F(1)).view(np.uint32))
    l1p = SG.sg_log1p_error(1, one, 4099, C.byref(worst))
    centres = [int(np.array(F(2.0 ** ex)).view(np.uint32)) for ex in range(-126, 1)] + [L1P_WORST_BITS, 1 + 2048]
    for c in centres:
        l1p = max(l1p, SG.sg_log1p_error(max(1, c - 2048), min(one, c + 2048), 1, C.byref(worst)))
    below = C.c_double(0)
    lo, hi = 0x80000000, int(np.array(F(-90)).view(np.uint32))
    sp = SG.sg_softplus_error(lo, hi, 4099, C.byref(worst), C.byref(below))
    centres = [int(np.array(F(-(2.0 ** ex))).view(np.uint32)) for ex in range(-126, 7)]
    centres += [int(np.array(F(-86)).view(np.uint32)), hi - 2048, SP_WORST_BITS]
    for c in centres:
        got = SG.sg_softplus_error(max(lo, c - 2048), min(hi, c + 2048), 1, C.byref(worst), C.byref(below))
        assert got >= 0                                                  # (-1: a nonzero result below the floor)
        sp = max(sp, got)
    print("Log1pUnit %.6f ulp (recorded %.4f), softplus %.6f ulp (recorded %.4f), below the floor <= %.4g"
          % (l1p, ref.E_L1P, sp, ref.E_SP, below.value))
    assert 0 < l1p <= ref.E_L1P and 0 < sp <= ref.E_SP
    assert 0 < below.value <= ref.SP_BELOW < 2.0 ** -124
    # the recorded worst cases are reproduced to the digits recorded
    assert abs(SG.sg_log1p_error(L1P_WORST_BITS, L1P_WORST_BITS, 1, C.byref(worst)) - ref.E_L1P) < 1e-4
    assert abs(SG.sg_softplus_error(SP_WORST_BITS, SP_WORST_BITS, 1, C.byref(worst), C.byref(below)) - ref.E_SP) < 1e-4


def test_rank_tie_rule_against_the_double_argsort():
    """negatives equal to the positive, an earlier positive equal to the last, K = 0: rank_of ==
    the literal mrr_score restatement on concat([neg, pos]) with the earlier positives counted as
    the reference would count more negatives"""
    x = np.array([[1.0, 1.0, 0.5, 2.0, 1.0, -3.0],          # P = 1: two ties and one above
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],           # all equal: every tie goes against it
                  [5.0, 1.0, 2.0, 3.0, 4.0, 4.5],           # the best
                  [-2.0, 1.0, -2.0, 3.0, -2.5, -2.0]], F)
    got = ref.rank_of(x, 1)
    assert np.array_equal(got, ref.mrr_score_ranks(x[:, :1], x[:, 1:])) and got.tolist() == [3, 5, 0, 4]
    # P = 2: the last positive is column 1; the earlier positive (column 0) counts like a negative
    got = ref.rank_of(x, 2)
    others = np.concatenate([x[:, 2:], x[:, :1]], 1)
    assert np.array_equal(got, ref.mrr_score_ranks(x[:, 1:2], others)) and got.tolist() == [3, 5, 5, 1]
    assert ref.rank_of(x[:, :1], 1).tolist() == [0, 0, 0, 0]             # K = 0
    assert ref.mrr_score_ranks(x[:, :1], x[:, :0]).tolist() == [0, 0, 0, 0]
    assert ref.metric("mrr", [0, 1, 3]) == (1 + 0.5 + 0.25) / 3 and ref.metric("mr", [0, 1, 3]) == 7 / 3
    assert ref.metric("hit1", [0, 1, 3]) == 1 / 3 and ref.metric("hit3", [0, 1, 3]) == 2 / 3


def test_rank_ties_through_the_host_build(SG):
    """rows that make equal logits exactly: small integers, so every dot product is exact"""
    rng = np.random.default_rng(21)
    d = 8
    target = placed(rng.integers(-3, 4, (6, d)).astype(F))
    context = placed(rng.integers(-3, 4, (9, d)).astype(F))
    context[1] = context[0]                                              # equal logits under every src
    context[2] = context[0]
    src = np.array([0, 1, 2, 3, 4, 5])
    pos = np.array([[0, 1]] * 6)                                         # an earlier positive equal to the last
    neg = np.array([[2, 0, 3, 4, 5]] * 6)                                # two negatives equal to it
    (logits, rank, _, _), _ = check_both(SG, target, context, src, pos, neg, rng)
    assert np.all(logits[:, 0] == logits[:, 1]) and np.all(logits[:, 2] == logits[:, 1])
    want = ref.mrr_score_ranks(logits[:, 1:2], np.concatenate([logits[:, 2:], logits[:, :1]], 1))
    assert np.array_equal(rank, want) and np.all(rank >= 3)
    (_, rank0, _, _), _ = check_both(SG, target, context, src, pos, None, rng)
    assert rank0.tolist() == [1] * 6                                     # K = 0, P = 2: the tie alone
    (_, rank1, _, _), _ = check_both(SG, target, context, src, pos[:, :1], None, rng)
    assert rank1.tolist() == [0] * 6                                     # K = 0, P = 1


def test_ids_that_name_no_row(SG):
    """-1, rows + 3 and 2^33 + 5 in src, pos and neg: never read, a row of zeros, a term of ln 2 in
    the loss and zero gradient rows"""
    rng = np.random.default_rng(11)
    d, rows_t, rows_c = 20, 40, 37
    target, context = tables(rng, d)
    bad_t, bad_c = [-1, rows_t + 3, (1 << 33) + 5], [-1, rows_c + 3, (1 << 33) + 5]
    src, pos, neg = batch(rng, 12, 2, 5, rows_t, rows_c)
    src[0:3] = bad_t
    pos[3:6, 1] = bad_c
    neg[6, 0:3] = bad_c
    neg[0, 4] = -1                                                       # beside a bad src
    (logits, rank, row_loss, loss), (gs, gp, gn) = check_both(SG, target, context, src, pos, neg, rng)
    zero = np.zeros(d, F)
    assert not logits[0:3].any() and not logits[3:6, 1].any() and not logits[6, 2:5].any()
    seven = LN2
    for _ in range(6):
        seven = seven + LN2
    assert all(row_loss[i] == seven for i in range(3))                   # 7 terms of ln 2, added one by one
    assert all(same(gs[i], zero) for i in range(3)) and all(same(gp[i, 1], zero) for i in range(3, 6))
    assert all(same(gn[6, j], zero) for j in range(3)) and same(gn[0, 4], zero)
    assert gs[3:].any(1).all() and gn[6, 3:].any() and gp[3:6, 0].any()
    # a bad id is a row of zeros: the same loss as tables with a zero row at that id
    t0 = placed(np.concatenate([target, np.zeros((1, d), F)]))
    c0 = placed(np.concatenate([context, np.zeros((1, d), F)]))
    fix = lambda ids, rows: np.where((ids >= 0) & (ids < rows), ids, rows)               # noqa: E731
    again = run(SG, t0, c0, fix(src, rows_t), fix(pos, rows_c), fix(neg, rows_c))
    assert same(again[0], logits) and same(again[2], row_loss) and same(F(again[3]), F(loss))
    assert np.array_equal(again[1], rank)


def test_repeated_ids_scatter_in_occurrence_order(SG):
    rng = np.random.default_rng(15)
    target, context = tables(rng, 64)
    src = np.array([4, 9, 4])
    pos = np.array([[5], [9], [6]])
    neg = np.array([[5, 5, 7], [9, 1, 9], [6, 5, 5]])
    _, (gs, gp, gn) = check_both(SG, target, context, src, pos, neg, rng)
    keys = np.concatenate([pos.reshape(-1), neg.reshape(-1)])
    rows = np.concatenate([gp.reshape(-1, 64), gn.reshape(-1, 64)])
    table = ref.scatter_rows(rows, keys, 37)
    assert same(table[5], (((gp[0, 0] + gn[0, 0]) + gn[0, 1]) + gn[2, 1]) + gn[2, 2])
    assert same(ref.scatter_rows(gs, src, 40)[4], gs[0] + gs[2])


def test_restatement_within_the_derived_bound_of_float64(capsys):
    """|fp32 restatement - float64 formulation| <= the bounds derived in skipgram_ref.py, no
    margin: the loss, and the three gradient blocks; rows uniform in [-1, 1]"""
    worst_l = worst_g = 0.0
    for d in ref.DIMS:
        rng = np.random.default_rng(1000 + d)
        target, context = tables(rng, d, 300, 280, scale=False)
        src, pos, neg = batch(rng, 90, 2, 5, 300, 280)
        src[3], pos[4, 0], neg[5, 2] = -1, 283, (1 << 33) + 5
        for v in {1, ref.chunk_width(d, 0, 4, 0, 4)}:
            logits, _, _, loss = ref.forward(target, context, src, pos, neg, v)
            x64, dx, loss64, bound = ref.forward64(target, context, src, pos, neg)
            assert np.all(np.abs(logits.astype(np.float64) - x64) <= dx), (d, v)
            err = abs(float(loss) - loss64)
            assert err <= bound, (d, v, err / bound)
            worst_l = max(worst_l, err / bound)
            g = 1.7
            got = ref.grad(target, context, src, pos, neg, logits, g)
            for a, (w, dw), name in zip(got, ref.grad64(target, context, src, pos, neg, g), ("src", "pos", "neg")):
                err = np.abs(a.astype(np.float64) - w)
                assert np.all(err <= dw), (d, v, name, float((err / np.maximum(dw, 1e-300)).max()))
                worst_g = max(worst_g, float((err / np.maximum(dw, 1e-300)).max()))
    with capsys.disabled():
        print("\n[skipgram_loss] worst error / bound: loss %.4f, gradient rows %.4f" % (worst_l, worst_g))
    assert 0 < worst_l <= 1 and 0 < worst_g <= 1


def test_new_entries_are_exported_and_bound():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    for name, n_args in (("euler_gpu_skipgram_loss", 18), ("euler_gpu_skipgram_loss_grad", 19)):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
        assert name + "(" in hdr
        assert len(_lib.SIGNATURES[name][1]) == n_args


def test_sources_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "$(HERE)skipgram.h" in mk and "skipgram_kernels.hip" in mk


def test_op_is_public():
    from euler_amd import ops
    assert callable(ops.skipgram_loss) and callable(ops.rank_metric)
