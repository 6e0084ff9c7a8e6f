"""The arithmetic of triple scoring with TransR's matrix projection (euler_amd/csrc/kg_matrix.h),
compiled with the host compiler, against the numpy restatement tests/triple_score_matrix_ref.py:
bit equality of the forward and of every gradient block (the per-occurrence rows, the gz rows and
the ordered matrix gradient), the corner cases, the restatement in float64 against the torch
float64 autograd composition of the reference's expressions, and the fp32 restatement within the
derived bound of float64.  CPU only.  Also: the new C-ABI entries are exported and bound."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import triple_score_matrix_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
KINDS, CORRUPTS = ("trans_l1", "trans_l2"), ("front", "tail", "both")
NAMES = ("src", "rel", "dst", "neg", "gz_src", "gz_dst", "gz_neg", "matrix")
ENT_ROWS, REL_ROWS = 40, 5


@pytest.fixture(scope="module")
def KG():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libkg_matrix_check.so")
    src = os.path.join(HERE, "csrc", "kg_matrix_check.cc")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", h)
                    for h in ("kg_matrix.h", "kg_score.h", "mp_weighted.h", "sparse_embed.h", "half_cvt.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # the host compiler alone, no HIP header; -ffp-contract=off as the library's build
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    L.kg_matrix_chunk_width.argtypes = [C.c_int64, f32p]
    L.kg_matrix_chunk_width.restype = C.c_int
    L.kg_matrix_triple.argtypes = [C.c_int32] * 3 + [f32p, C.c_int64, C.c_int64, f32p, C.c_int64, C.c_int64, f32p,
                                                     i64p, i64p, i64p, i64p, C.c_int64, C.c_int64] + [f32p] * 12
    L.kg_matrix_triple.restype = C.c_int
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


class Tables(object):
    """ent [ent_rows, de], rel [rel_rows, dr], matrix [rel_rows, de * dr] -> (ent, rel, matrix)"""

    def __init__(self, rng, de, dr, ent_rows=ENT_ROWS, rel_rows=REL_ROWS, shift=0, wide=True):
        def draw(rows, d, scale):
            x = (rng.random((rows, d)) * 2 - 1) * scale
            if wide:
                x = x * 10.0 ** rng.integers(-2, 3, (rows, d))
            return placed(x.astype(np.float32), shift)
        self.ent, self.rel, self.matrix = draw(ent_rows, de, 4), draw(rel_rows, dr, 4), draw(rel_rows, de * dr, 1)
        self.all = (self.ent, self.rel, self.matrix)


def width(tabs):
    return ref.matrix_chunk_width(tabs[1].shape[1], tabs[1].ctypes.data, 4)


def batch(rng, b, k, ent_rows=ENT_ROWS, rel_rows=REL_ROWS):
    src, dst = rng.integers(0, ent_rows, b), rng.integers(0, ent_rows, b)
    rel_id = rng.integers(0, rel_rows, b)
    neg = rng.integers(0, ent_rows, (b, k)) if k else None
    return src, rel_id, dst, neg


def run(L, tabs, src, rel_id, dst, neg, kind, corrupt, v=0, g_pos=None, g_neg=None):
    """the host build: forward -> (pos, neg_out); with g_pos the gradient -> the eight blocks of NAMES"""
    ent, rel, matrix = tabs
    b, de, dr = len(src), ent.shape[1], rel.shape[1]
    k = 0 if neg is None else neg.shape[1]
    kp = 2 * k if corrupt == "both" else k
    src, rel_id, dst = (np.ascontiguousarray(x, np.int64) for x in (src, rel_id, dst))
    neg = None if neg is None else np.ascontiguousarray(neg, np.int64)
    head = (ref.KIND[kind], ref.CORRUPT[corrupt], v, fp(ent), ent.shape[0], de, fp(rel), rel.shape[0], dr, fp(matrix),
            ip(src), ip(rel_id), ip(dst), ip(neg), b, k)
    if g_pos is None:
        pos, out = np.full(b, np.nan, np.float32), np.full((b, kp), np.nan, np.float32)
        assert L.kg_matrix_triple(*head, fp(pos), fp(out), *([None] * 10)) == 0
        return pos, out
    g_pos = np.ascontiguousarray(g_pos, np.float32)
    g_neg = None if g_neg is None else np.ascontiguousarray(g_neg, np.float32)
    nan = lambda *shape: np.full(shape, np.nan, np.float32)                             # noqa: E731
    gs, gr, gd, gn = nan(b, de), nan(b, dr), nan(b, de), nan(b, k, de)
    zs, zd, zn, gm = nan(b, dr), nan(b, dr), nan(b, k, dr), nan(rel.shape[0], de * dr)
    assert L.kg_matrix_triple(*head, None, None, fp(g_pos), fp(g_neg), fp(gs), fp(gr), fp(gd), fp(gn), fp(zs),
                              fp(zd), fp(zn), fp(gm)) == 0
    return gs, gr, gd, gn, zs, zd, zn, gm


def same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


def want_grad(tabs, src, rel_id, dst, neg, kind, corrupt, v, g_pos, g_neg, dt=np.float32):
    rows = ref.grad(*tabs, src, rel_id, dst, neg, kind, corrupt, v, g_pos, g_neg, dt=dt)
    gm = ref.matrix_grad(tabs[0], tabs[1].shape[0], src, rel_id, dst, neg, rows[4], rows[5], rows[6], dt=dt)
    return rows + (gm,)


def check_both(L, tabs, src, rel_id, dst, neg, kind, corrupt, rng, v=0):
    """forward and gradient bits of the host build == the restatement; -> the gradient blocks"""
    b = len(src)
    k = 0 if neg is None else neg.shape[1]
    kp = 2 * k if corrupt == "both" else k
    vv = v or width(tabs)
    assert v or vv == L.kg_matrix_chunk_width(tabs[1].shape[1], fp(tabs[1]))
    tag = (kind, corrupt, k, vv)
    pos, out = run(L, tabs, src, rel_id, dst, neg, kind, corrupt, v)
    want_pos, want_out = ref.forward(*tabs, src, rel_id, dst, neg, kind, corrupt, vv)
    assert same(pos, want_pos) and same(out, want_out), tag
    g_pos = (rng.random(b) * 2 - 1).astype(np.float32)
    g_neg = (rng.random((b, kp)) * 2 - 1).astype(np.float32) if k else None
    got = run(L, tabs, src, rel_id, dst, neg, kind, corrupt, v, g_pos, g_neg)
    want = want_grad(tabs, src, rel_id, dst, neg, kind, corrupt, vv, g_pos, g_neg)
    for g, w, name in zip(got, want, NAMES):
        assert same(g, w), tag + (name,)
    return got


@pytest.mark.parametrize("de,dr", ref.DIMS + ((8, 512), (512, 24)))
def test_host_build_equals_the_restatement(KG, de, dr):
    """V = 1 / 4 / 8 by dr, one to eight chunks a lane, every butterfly width; 2 kinds x 3 corrupt
    modes x K in {0, 1, 5}; B = 11, 40 entity rows, 5 relation rows (one of them unused)"""
    rng = np.random.default_rng(100 + 7 * de + dr)
    t = Tables(rng, de, dr)
    for k in (0, 1, 5):
        src, rel_id, dst, neg = batch(rng, 11, k, rel_rows=REL_ROWS - 1)
        for kind in KINDS:
            for corrupt in (CORRUPTS if k else ("both",)):
                got = check_both(KG, t.all, src, rel_id, dst, neg, kind, corrupt, rng)
                assert same(got[7][REL_ROWS - 1], np.zeros(de * dr, np.float32))     # no triple: +0


@pytest.mark.parametrize("de,dr", [(5, 8), (24, 64), (7, 512)])
def test_unaligned_rel_and_forced_widths(KG, de, dr):
    """rel one element past a 16-byte boundary takes V = 1; the other tables do not count; V in
    {1, 4, 8} forced"""
    rng = np.random.default_rng(7 + dr)
    t, t0 = Tables(rng, de, dr, shift=1), Tables(rng, de, dr)
    src, rel_id, dst, neg = batch(rng, 9, 5)
    assert width(t.all) == 1 == KG.kg_matrix_chunk_width(dr, fp(t.rel)) and width(t0.all) == 8
    mixed = (t.ent, t0.rel, t.matrix)
    assert width(mixed) == 8 == KG.kg_matrix_chunk_width(dr, fp(t0.rel))
    for kind in KINDS:
        check_both(KG, t.all, src, rel_id, dst, neg, kind, "both", rng)
        check_both(KG, mixed, src, rel_id, dst, neg, kind, "both", rng)
        for v in (1, 4, 8):
            check_both(KG, t.all, src, rel_id, dst, neg, kind, "both", rng, v=v)
    assert ref.matrix_chunk_width(dr, 16, 2) == 8 and ref.matrix_chunk_width(dr, 8, 2) == 4
    assert ref.matrix_chunk_width(dr, 8, 4) == 1 and ref.matrix_chunk_width(dr, 2, 2) == 1


@pytest.mark.parametrize("kind", KINDS)
def test_ids_that_name_no_row(KG, kind):
    """-1, rows + 3 and 2^33 + 5 in every id column: never read, rows of zeros, zero gradient
    rows, no term in the matrix gradient; a rel_id removes rel[rho] and M_rho; the scores of
    tables with a zero row appended"""
    rng = np.random.default_rng(11)
    de, dr = 12, 20
    t = Tables(rng, de, dr)
    bad_e, bad_r = [-1, ENT_ROWS + 3, (1 << 33) + 5], [-1, REL_ROWS + 3, (1 << 33) + 5]
    src, rel_id, dst, neg = batch(rng, 12, 5)
    src[0:3], dst[3:6], rel_id[6:9] = bad_e, bad_e, bad_r
    neg[9, 0:3] = bad_e
    neg[0, 4] = -1                                            # beside a bad src
    gs, gr, gd, gn, zs, zd, zn, gm = check_both(KG, t.all, src, rel_id, dst, neg, kind, "both", rng)
    ze, zr = np.zeros(de, np.float32), np.zeros(dr, np.float32)
    assert all(same(gs[i], ze) for i in range(3)) and all(same(gd[i], ze) for i in range(3, 6))
    assert all(same(gr[i], zr) for i in range(6, 9))
    assert all(not gs[i].any() and not gd[i].any() and not gn[i].any() for i in range(6, 9))   # M_rho removed
    assert all(same(gn[9, j], ze) for j in range(3)) and same(gn[0, 4], ze)
    assert gs[3:6].any() and gn[9, 3:].any() and gr[:6].any() and gm.any()
    # a bad id is a row of zeros: the same scores as tables with a zero row (a zero matrix) at that id
    pad = lambda x, d: placed(np.concatenate([x, np.zeros((1, d), np.float32)]))          # noqa: E731
    fix = lambda ids: np.where((ids >= 0) & (ids < ENT_ROWS), ids, ENT_ROWS)              # noqa: E731
    rfix = np.where((rel_id >= 0) & (rel_id < REL_ROWS), rel_id, REL_ROWS)
    pos, out = run(KG, t.all, src, rel_id, dst, neg, kind, "both")
    padded = (pad(t.ent, de), pad(t.rel, dr), pad(t.matrix, de * dr))
    pos0, out0 = run(KG, padded, fix(src), rfix, fix(dst), fix(neg), kind, "both")
    assert same(pos, pos0) and same(out, out0)


@pytest.mark.parametrize("kind", KINDS)
def test_projected_row_with_z_zero(KG, kind):
    """an all-zero entity row, an all-zero matrix (z = 0) and rows of 1e-8 (ss under the clamp):
    inv = 1 / sqrt(1e-12f), gz = inv * gy; everything finite"""
    rng = np.random.default_rng(16)
    t = Tables(rng, 6, 8)
    t.ent[3] = 0
    t.ent[4] = np.float32(1e-8)
    t.matrix[2] = 0
    t.rel[1] = 0
    src, rel_id, dst = np.array([3, 0, 4, 3, 5]), np.array([0, 1, 2, 1, 2]), np.array([1, 3, 3, 4, 6])
    neg = np.array([[3, 5], [4, 3], [6, 3], [3, 4], [7, 8]])
    got = check_both(KG, t.all, src, rel_id, dst, neg, kind, "both", rng)
    assert all(np.isfinite(g).all() for g in got) and got[0][1].any()
    pos, out = run(KG, t.all, src, rel_id, dst, neg, kind, "both")
    assert np.isfinite(pos).all() and np.isfinite(out).all()
    assert not got[0][4].any() and not got[3][4].any() and got[4][4].any()       # M = 0: gx = 0, gz is not


def test_zero_l2_norm_has_zero_gradients(KG):
    """src == dst and r a zero row, trans_l2: q == 0 and every gradient of the triple is 0, not NaN"""
    rng = np.random.default_rng(14)
    t = Tables(rng, 9, 20)
    t.rel[2] = 0
    src, rel_id, dst, neg = np.array([7, 7]), np.array([2, 2]), np.array([7, 8]), np.array([[7], [9]])
    pos, out = run(KG, t.all, src, rel_id, dst, neg, "trans_l2", "both")
    assert pos[0] == 0 and out[0, 0] == 0 and out[0, 1] == 0 and pos[1] != 0
    got = check_both(KG, t.all, src, rel_id, dst, neg, "trans_l2", "both", rng)
    assert all(not g[0].any() for g in got[:7])
    assert all(np.isfinite(g).all() for g in got) and got[0][1].any()


def test_sign_of_a_zero_residual_is_zero(KG):
    """trans_l1 with src == dst and r a zero row: every e_j is 0, sign(0) = 0, the gradients of the
    true triple's rows are +0"""
    rng = np.random.default_rng(15)
    t = Tables(rng, 9, 20)
    t.rel[2] = 0
    src, rel_id, dst = np.array([7, 7]), np.array([2, 2]), np.array([7, 8])
    got = check_both(KG, t.all, src, rel_id, dst, None, "trans_l1", "both", rng)
    assert all(not g[0].any() for g in got[:7]) and got[0][1].any()


@pytest.mark.parametrize("kind", KINDS)
def test_matrix_gradient_order_and_repeats(KG, kind):
    """n == src and repeated triples on one relation: the matrix gradient takes every occurrence,
    in triple order and within a triple n_0 .. n_{K-1}, h, t"""
    rng = np.random.default_rng(17)
    de, dr = 4, 8
    t = Tables(rng, de, dr)
    src, rel_id, dst = np.array([4, 9, 4]), np.array([1, 0, 1]), np.array([5, 9, 6])
    neg = np.array([[4, 7], [9, 1], [6, 4]])
    gs, gr, gd, gn, zs, zd, zn, gm = check_both(KG, t.all, src, rel_id, dst, neg, kind, "both", rng)
    x = t.ent
    outer = lambda i, gz: x[i][:, None] * gz[None, :]                                   # noqa: E731
    want = outer(4, zn[0, 0])
    for term in (outer(7, zn[0, 1]), outer(4, zs[0]), outer(5, zd[0]), outer(6, zn[2, 0]), outer(4, zn[2, 1]),
                 outer(4, zs[2]), outer(6, zd[2])):
        want = want + term
    assert same(gm[1], want.reshape(-1))


# ---- float64: the restatement against the torch autograd composition --------------------------
def composition64(torch, tabs, src, rel_id, dst, neg, kind, corrupt):
    """generate_embedding and calculate_scores as the reference spells them (transR.py:41-68,
    transX.py:105-133), in torch float64: the lookup of one [de, dr] matrix per triple, its tile
    over the negatives, matmul, tf.nn.l2_normalize, the norms, the concat"""
    ent, rel, matrix = tabs
    eps = float(np.float32(1e-12))
    k, de, dr = neg.shape[1], ent.shape[1], rel.shape[1]

    def l2n(x):
        return x * torch.rsqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=eps))

    m = matrix[rel_id].reshape(-1, 1, de, dr)                                   # [B, 1, de, dr]
    project = lambda x, mm: l2n(torch.matmul(x.unsqueeze(-2), mm).squeeze(-2))          # noqa: E731
    h, t = project(ent[src].unsqueeze(1), m), project(ent[dst].unsqueeze(1), m)
    n = project(ent[neg], m.repeat(1, k, 1, 1))
    r = l2n(rel[rel_id].unsqueeze(1))

    def score(a, r, c):
        return -torch.linalg.norm(a + r - c, ord=1 if kind == "trans_l1" else 2, dim=-1)

    hh, rr, tt = h.repeat(1, k, 1), r.repeat(1, k, 1), t.repeat(1, k, 1)
    front, tail = score(n, rr, tt), score(hh, rr, n)
    out = front if corrupt == "front" else tail if corrupt == "tail" else torch.cat([front, tail], 1)
    return score(h, r, t).reshape(-1), out


def close64(a, b):
    """the project's criterion for two float64 forms (tests/test_triple_score_gpu.py)"""
    return np.all(np.abs(a - b) <= 1e-9 * (1 + np.abs(b)))


@pytest.mark.parametrize("kind", KINDS)
def test_float64_restatement_equals_the_torch_autograd_composition(kind):
    """forward and the gradients of all three tables; random rows, src != dst and no id out of
    range, so no trans_l1 residual is exactly 0 and no trans_l2 norm is 0"""
    import torch
    for (de, dr), corrupt in (((3, 5), "both"), ((20, 12), "front"), ((33, 64), "tail")):
        rng = np.random.default_rng(500 + de)
        t = Tables(rng, de, dr, wide=False)
        b, k = 11, 5
        src, rel_id, _, neg = batch(rng, b, k)
        dst = (src + 1 + rng.integers(0, ENT_ROWS - 2, b)) % ENT_ROWS
        kp = 2 * k if corrupt == "both" else k
        g_pos, g_neg = rng.random(b) * 2 - 1, rng.random((b, kp)) * 2 - 1
        pos, out = ref.forward(*t.all, src, rel_id, dst, neg, kind, corrupt, 1, dt=np.float64)
        gs, gr, gd, gn, zs, zd, zn, gm = want_grad(t.all, src, rel_id, dst, neg, kind, corrupt, 1, g_pos, g_neg,
                                                   dt=np.float64)
        tt = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in t.all]
        ids = [torch.from_numpy(np.asarray(x, np.int64)) for x in (src, rel_id, dst, neg)]
        p64, o64 = composition64(torch, tt, *ids, kind, corrupt)
        assert close64(pos, p64.detach().numpy()) and close64(out, o64.detach().numpy()), (de, "forward")
        ((p64 * torch.from_numpy(g_pos)).sum() + (o64 * torch.from_numpy(g_neg)).sum()).backward()
        keys = np.concatenate([src, dst, neg.reshape(-1)])
        want = (ref.scatter_rows(np.concatenate([gs, gd, gn.reshape(-1, de)]), keys, ENT_ROWS),
                ref.scatter_rows(gr, rel_id, REL_ROWS), gm)
        for i, table in enumerate(want):
            assert table.any() and close64(table, tt[i].grad.numpy()), (de, "table", i)


# ---- the fp32 restatement within the derived bound of float64 ---------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_within_the_derived_bound_of_float64(kind, capsys):
    """|fp32 restatement - float64| <= gamma(de + 2 dr + 4 | 6) * (the float64 sum of the magnitudes
    of the terms, which carry the projection's cancellation kappa), no margin - the derivation is
    in triple_score_matrix_ref: the de-term projection sum perturbs z by gamma(de) Z absolutely,
    the normalisation turns that into gamma(de) Y, itself adds gamma(dr + 3), the residual two
    roundings more, the score's sum gamma(dr - 1) (l1) or the root gamma(dr + 1) (l2).  Rows
    uniform in [-4, 4], matrix elements in [-1, 1]."""
    worst = 0.0
    for de, dr in ref.DIMS:
        rng = np.random.default_rng(1000 + 7 * de + dr)
        t = Tables(rng, de, dr, ent_rows=300, rel_rows=7, wide=False)
        src, rel_id, dst, neg = batch(rng, 90, 5, 300, 7)
        for v in {1, width(t.all)}:
            pos, out = ref.forward(*t.all, src, rel_id, dst, neg, kind, "both", v)
            p64, o64, mp, mo = ref.forward64(*t.all, src, rel_id, dst, neg, kind, "both")
            for got, want, mag in ((pos, p64, mp), (out, o64, mo)):
                err, bound = np.abs(got.astype(np.float64) - want), ref.forward_bound(kind, de, dr, mag)
                known = np.isfinite(bound)
                assert known.mean() > 0.9 and np.all(err[known] <= bound[known]), \
                    (de, dr, v, float((err[known] / bound[known]).max()))
                worst = max(worst, float((err[known] / np.maximum(bound[known], 1e-300)).max()))
    with capsys.disabled():
        print("\n[triple_score_matrix %s] worst error / bound = %.4f" % (kind, worst))
    assert 0 < worst <= 1


# ---- plumbing ---------------------------------------------------------------------------------
def test_new_entries_are_exported_and_bound():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    for name, n_args in (("euler_gpu_triple_score_matrix", 22), ("euler_gpu_triple_score_matrix_grad", 33)):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
        assert name + "(" in hdr
        assert len(_lib.SIGNATURES[name][1]) == n_args


def test_sources_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "$(HERE)kg_matrix.h" in mk and "kg_matrix_kernels.hip" in mk


def test_op_is_public():
    from euler_amd import ops
    assert callable(ops.triple_score_matrix)
