"""The per-lane arithmetic of the fused triple scoring (euler_amd/csrc/kg_score.h), compiled with
the host compiler, against the numpy restatement tests/triple_score_ref.py: bit equality of the
forward and the gradient, the corner cases, and the restatement within the derived bound of the
float64 formulation.  CPU only.  Also: the new C-ABI entries are exported and bound."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import triple_score_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
KINDS, CORRUPTS = ("trans_l1", "trans_l2", "distmult"), ("front", "tail", "both")


@pytest.fixture(scope="module")
def KG():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libkg_score_check.so")
    src = os.path.join(HERE, "csrc", "kg_score_check.cc")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", h)
                    for h in ("kg_score.h", "mp_weighted.h", "sparse_embed.h", "half_cvt.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # the host compiler alone, no HIP header; -ffp-contract=off as the library's build
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    L.kg_chunk_width.argtypes = [C.c_int64, f32p, f32p]
    L.kg_chunk_width.restype = C.c_int
    L.kg_triple.argtypes = [C.c_int32] * 4 + [f32p, C.c_int64, f32p, C.c_int64, i64p, i64p, i64p, i64p,
                                              C.c_int64, C.c_int64, C.c_int64] + [f32p] * 8
    L.kg_triple.restype = C.c_int
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


def run(L, ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize, v=0, g_pos=None, g_neg=None):
    """the host build: forward -> (pos, neg_out); with g_pos the gradient -> the four row blocks"""
    b, d = len(src), ent.shape[1]
    k = 0 if neg is None else neg.shape[1]
    kp = 2 * k if corrupt == "both" else k
    src, rel_id, dst = (np.ascontiguousarray(x, np.int64) for x in (src, rel_id, dst))
    neg = None if neg is None else np.ascontiguousarray(neg, np.int64)
    head = (ref.KIND[kind], int(normalize), ref.CORRUPT[corrupt], v, fp(ent), ent.shape[0], fp(rel), rel.shape[0],
            ip(src), ip(rel_id), ip(dst), ip(neg), b, k, d)
    if g_pos is None:
        pos, out = np.full(b, np.nan, np.float32), np.full((b, kp), np.nan, np.float32)
        assert L.kg_triple(*head, fp(pos), fp(out), None, None, None, None, None, None) == 0
        return pos, out
    g_pos = np.ascontiguousarray(g_pos, np.float32)
    g_neg = None if g_neg is None else np.ascontiguousarray(g_neg, np.float32)
    gs, gr, gd = (np.full((b, d), np.nan, np.float32) for _ in range(3))
    gn = np.full((b, k, d), np.nan, np.float32)
    assert L.kg_triple(*head, None, None, fp(g_pos), fp(g_neg), fp(gs), fp(gr), fp(gd), fp(gn)) == 0
    return gs, gr, gd, gn


def same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


def tables(rng, d, ent_rows=40, rel_rows=5, shift=0):
    ent = placed(((rng.random((ent_rows, d)) * 8 - 4) * 10.0 ** rng.integers(-2, 3, (ent_rows, d))).astype(np.float32),
                 shift)
    rel = placed((rng.random((rel_rows, d)) * 8 - 4).astype(np.float32), shift)
    return ent, rel


def batch(rng, b, k, ent_rows, rel_rows):
    src, dst = rng.integers(0, ent_rows, b), rng.integers(0, ent_rows, b)
    rel_id = rng.integers(0, rel_rows, b)
    neg = rng.integers(0, ent_rows, (b, k)) if k else None
    return src, rel_id, dst, neg


def check_both(L, ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize, rng, v=0):
    """forward and gradient bits of the host build == the restatement; -> the gradient rows"""
    b = len(src)
    k = 0 if neg is None else neg.shape[1]
    kp = 2 * k if corrupt == "both" else k
    vv = v or ref.chunk_width(ent.shape[1], ent.ctypes.data, 4, rel.ctypes.data, 4)
    assert v or vv == L.kg_chunk_width(ent.shape[1], fp(ent), fp(rel))
    tag = (kind, corrupt, normalize, k, vv)
    pos, out = run(L, ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize, v)
    want_pos, want_out = ref.forward(ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize, vv)
    assert same(pos, want_pos) and same(out, want_out), tag
    g_pos = (rng.random(b) * 2 - 1).astype(np.float32)
    g_neg = (rng.random((b, kp)) * 2 - 1).astype(np.float32) if k else None
    got = run(L, ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize, v, g_pos, g_neg)
    want = ref.grad(ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize, vv, g_pos, g_neg)
    for g, w, name in zip(got, want, ("src", "rel", "dst", "neg")):
        assert same(g, w), tag + (name,)
    return got


@pytest.mark.parametrize("d", ref.DIMS)
def test_host_build_equals_the_restatement(KG, d):
    """V = 1 / 4 / 8 by d, one and several chunks a lane, every butterfly width; 3 kinds x 3
    corrupt modes x normalize on / off x K in {0, 1, 5}"""
    rng = np.random.default_rng(100 + d)
    ent, rel = tables(rng, d)
    for k in (0, 1, 5):
        src, rel_id, dst, neg = batch(rng, 11, k, 40, 5)
        for kind in KINDS:
            for corrupt in (CORRUPTS if k else ("both",)):
                for normalize in (True, False):
                    check_both(KG, ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize, rng)


@pytest.mark.parametrize("d", [8, 64, 520])
def test_unaligned_table_start_and_forced_widths(KG, d):
    """tables one element past a 16-byte boundary take V = 1; the 16-bit tables' V = 4 at d % 8 == 0"""
    rng = np.random.default_rng(7 + d)
    ent, rel = tables(rng, d, shift=1)
    assert ref.chunk_width(d, ent.ctypes.data, 4, rel.ctypes.data, 4) == 1 == KG.kg_chunk_width(d, fp(ent), fp(rel))
    assert ref.chunk_width(d, 8, 2, 16, 2) == 4 and ref.chunk_width(d, 16, 2, 32, 2) == 8
    assert ref.chunk_width(d, 8, 2, 16, 4) == 4 and ref.chunk_width(d, 8, 4, 16, 2) == 1
    src, rel_id, dst, neg = batch(rng, 9, 5, 40, 5)
    for kind in KINDS:
        check_both(KG, ent, rel, src, rel_id, dst, neg, kind, "both", True, rng)
        for v in (1, 4, 8):
            check_both(KG, ent, rel, src, rel_id, dst, neg, kind, "both", True, rng, v=v)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("normalize", [True, False])
def test_ids_that_name_no_row(KG, kind, normalize):
    """-1, rows + 3 and 2^33 + 5 in every id column: never read, rows of zeros, zero gradient rows"""
    rng = np.random.default_rng(11)
    d, ent_rows, rel_rows = 20, 40, 5
    ent, rel = tables(rng, d)
    bad_e, bad_r = [-1, ent_rows + 3, (1 << 33) + 5], [-1, rel_rows + 3, (1 << 33) + 5]
    src, rel_id, dst, neg = batch(rng, 12, 5, ent_rows, rel_rows)
    src[0:3], dst[3:6], rel_id[6:9] = bad_e, bad_e, bad_r
    neg[9, 0:3] = bad_e
    neg[0, 4] = -1                                            # beside a bad src
    gs, gr, gd, gn = check_both(KG, ent, rel, src, rel_id, dst, neg, kind, "both", normalize, rng)
    zero = np.zeros(d, np.float32)
    assert all(same(gs[i], zero) for i in range(3)) and all(same(gd[i], zero) for i in range(3, 6))
    assert all(same(gr[i], zero) for i in range(6, 9)) and all(same(gn[9, j], zero) for j in range(3))
    assert same(gn[0, 4], zero) and gs[3:].any() and gn[9, 3:].any()
    # a bad id is a row of zeros: the same scores as a table with a zero row at that id
    ent0 = placed(np.concatenate([ent, np.zeros((1, d), np.float32)]))
    fix = lambda ids: np.where((ids >= 0) & (ids < ent_rows), ids, ent_rows)
    pos, out = run(KG, ent, rel, src, rel_id, dst, neg, kind, "both", normalize)
    rel0 = placed(np.concatenate([rel, np.zeros((1, d), np.float32)]))
    rfix = np.where((rel_id >= 0) & (rel_id < rel_rows), rel_id, rel_rows)
    pos0, out0 = run(KG, ent0, rel0, fix(src), rfix, fix(dst), fix(neg), kind, "both", normalize)
    assert same(pos, pos0) and same(out, out0)


@pytest.mark.parametrize("kind", KINDS)
def test_all_zero_row_under_normalize(KG, kind):
    """ss = 0 <= 1e-12: inv = 1 / sqrt(1e-12f), y = 0, and gx = inv * gy (no projection)"""
    rng = np.random.default_rng(12)
    d = 8
    ent, rel = tables(rng, d)
    ent[3] = 0
    ent[4] = np.float32(1e-8)                                 # ss = 8e-16: under the clamp too
    rel[1] = 0
    src, rel_id, dst = np.array([3, 0, 4, 3]), np.array([0, 1, 2, 1]), np.array([1, 3, 3, 4])
    neg = np.array([[3, 5], [4, 3], [6, 3], [3, 4]])
    gs, gr, gd, gn = check_both(KG, ent, rel, src, rel_id, dst, neg, kind, "both", True, rng)
    assert np.isfinite(gs).all() and np.isfinite(gn).all() and np.isfinite(gr).all() and gs[0].any()
    pos, out = run(KG, ent, rel, src, rel_id, dst, neg, kind, "both", True)
    assert np.isfinite(pos).all() and np.isfinite(out).all()


def test_sign_of_zero_residual(KG):
    """columns with h + r - t == 0 exactly: trans_l1 passes no gradient through them"""
    rng = np.random.default_rng(13)
    d = 8
    ent = placed(rng.integers(-8, 9, (6, d)).astype(np.float32))
    rel = placed(rng.integers(-8, 9, (2, d)).astype(np.float32))
    ent[1] = ent[0] + rel[0]
    ent[1, 5:] += 1                                           # columns 0..4 are exactly 0
    src, rel_id, dst, neg = np.array([0]), np.array([0]), np.array([1]), np.array([[2]])
    g_pos, g_neg = np.array([1.0], np.float32), np.zeros((1, 2), np.float32)
    gs, gr, gd, gn = run(KG, ent, rel, src, rel_id, dst, neg, "trans_l1", "both", False, 0, g_pos, g_neg)
    want = np.array([0] * 5 + [1] * 3, np.float32)            # e = -1 there: -sign(e) = +1
    assert same(gs[0], want) and same(gr[0], want) and same(gd[0], -want + 0) and not gn.any()
    check_both(KG, ent, rel, src, rel_id, dst, neg, "trans_l1", "both", False, rng)
    check_both(KG, ent, rel, src, rel_id, dst, neg, "trans_l1", "both", True, rng)


def test_zero_l2_norm_has_a_finite_gradient(KG):
    """src == dst and r a zero row, trans_l2 without normalize: q == 0 and the gradient is 0, not NaN"""
    rng = np.random.default_rng(14)
    d = 20
    ent, rel = tables(rng, d)
    rel[2] = 0
    src, rel_id, dst, neg = np.array([7, 7]), np.array([2, 2]), np.array([7, 8]), np.array([[7], [9]])
    pos, out = run(KG, ent, rel, src, rel_id, dst, neg, "trans_l2", "both", False)
    assert pos[0] == 0 and out[0, 0] == 0 and out[0, 1] == 0 and pos[1] != 0
    gs, gr, gd, gn = check_both(KG, ent, rel, src, rel_id, dst, neg, "trans_l2", "both", False, rng)
    assert not gs[0].any() and not gr[0].any() and not gd[0].any() and not gn[0].any()
    assert np.isfinite(gs).all() and gs[1].any()


@pytest.mark.parametrize("kind", KINDS)
def test_negative_equal_to_src(KG, kind):
    """n == src: the tail score of trans is s(h, r, h); its rows get separate gradient rows"""
    rng = np.random.default_rng(15)
    ent, rel = tables(rng, 64)
    src, rel_id, dst = np.array([4, 9, 4]), np.array([0, 1, 1]), np.array([5, 9, 6])
    neg = np.array([[4, 4, 7], [9, 1, 9], [6, 4, 5]])
    for normalize in (True, False):
        gs, gr, gd, gn = check_both(KG, ent, rel, src, rel_id, dst, neg, kind, "both", normalize, rng)
        assert gn[0, 0].any() and gs[0].any()
        # the table's gradient accumulates the occurrences in the stated order
        keys = np.concatenate([src, dst, neg.reshape(-1)])
        rows = np.concatenate([gs, gd, gn.reshape(-1, 64)])
        table = ref.scatter_rows(rows, keys, 40)
        assert same(table[4], ((gs[0] + gs[2]) + gn[0, 0] + gn[0, 1]) + gn[2, 1])


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_within_the_derived_bound_of_float64(kind, capsys):
    """|fp32 restatement - float64 formulation| <= gamma(n(kind, d)) * (the float64 sum of the
    magnitudes of the terms), no margin; rows uniform in [-4, 4]"""
    worst = 0.0
    for d in ref.DIMS:
        rng = np.random.default_rng(1000 + d)
        ent = (rng.random((300, d)) * 8 - 4).astype(np.float32)
        rel = (rng.random((7, d)) * 8 - 4).astype(np.float32)
        src, rel_id, dst, neg = batch(rng, 90, 5, 300, 7)
        for normalize in (True, False):
            for v in {1, ref.chunk_width(d, 0, 4, 0, 4)}:
                pos, out = ref.forward(ent, rel, src, rel_id, dst, neg, kind, "both", normalize, v)
                p64, o64, mp, mo = ref.forward64(ent, rel, src, rel_id, dst, neg, kind, "both", normalize)
                for got, want, mag in ((pos, p64, mp), (out, o64, mo)):
                    err, bound = np.abs(got.astype(np.float64) - want), ref.forward_bound(kind, d, mag)
                    assert np.all(err <= bound), (d, normalize, v, float((err / bound).max()))
                    worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    with capsys.disabled():
        print("\n[triple_score %s] worst error / bound = %.4f" % (kind, worst))
    assert 0 < worst <= 1


def test_new_entries_are_exported_and_bound():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    for name, n_args in (("euler_gpu_triple_score", 19), ("euler_gpu_triple_score_grad", 23)):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
        assert name + "(" in hdr
        assert len(_lib.SIGNATURES[name][1]) == n_args


def test_sources_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "$(HERE)kg_score.h" in mk and "kg_score_kernels.hip" in mk


def test_op_is_public():
    from euler_amd import ops
    assert callable(ops.triple_score)
