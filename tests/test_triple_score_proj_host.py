"""The per-lane arithmetic of triple scoring with the TransH / TransD projections
(euler_amd/csrc/kg_proj.h), compiled with the host compiler, against the numpy restatement
tests/triple_score_proj_ref.py: bit equality of the forward and of every gradient block, the
corner cases, the restatement in float64 against the torch float64 autograd composition of the
reference's expressions, and the fp32 restatement within the derived bound of float64.  CPU only.
Also: the new C-ABI entries are exported and bound."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import triple_score_proj_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
PROJS, KINDS, CORRUPTS = ("hyperplane", "transfer"), ("trans_l1", "trans_l2"), ("front", "tail", "both")
NAMES = ("src", "rel", "dst", "neg", "rel_aux", "src_aux", "dst_aux", "neg_aux")


@pytest.fixture(scope="module")
def KG():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libkg_proj_check.so")
    src = os.path.join(HERE, "csrc", "kg_proj_check.cc")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", h)
                    for h in ("kg_proj.h", "kg_score.h", "mp_weighted.h", "sparse_embed.h", "half_cvt.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        # the host compiler alone, no HIP header; -ffp-contract=off as the library's build
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    L.kg_proj_chunk_width.argtypes = [C.c_int64, f32p, f32p, f32p, f32p]
    L.kg_proj_chunk_width.restype = C.c_int
    L.kg_proj_triple.argtypes = [C.c_int32] * 4 + [f32p, f32p, C.c_int64, f32p, f32p, C.c_int64, i64p, i64p, i64p,
                                                   i64p, C.c_int64, C.c_int64, C.c_int64] + [f32p] * 12
    L.kg_proj_triple.restype = C.c_int
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
    """ent, ent_transfer [ent_rows, d] and rel, hyper, rel_transfer [rel_rows, d]; of(proj) gives
    (ent, ent_aux | None, rel, rel_aux)"""

    def __init__(self, rng, d, ent_rows=40, rel_rows=5, shift=0, wide=True):
        def draw(rows):
            x = rng.random((rows, d)) * 8 - 4
            if wide:
                x = x * 10.0 ** rng.integers(-2, 3, (rows, d))
            return placed(x.astype(np.float32), shift)
        self.ent = draw(ent_rows)
        self.ent_transfer = placed((rng.random((ent_rows, d)) * 2 - 1).astype(np.float32), shift)
        self.rel, self.hyper = draw(rel_rows), draw(rel_rows)
        self.rel_transfer = placed((rng.random((rel_rows, d)) * 2 - 1).astype(np.float32), shift)

    def of(self, proj):
        if proj == "hyperplane":
            return self.ent, None, self.rel, self.hyper
        return self.ent, self.ent_transfer, self.rel, self.rel_transfer


def width(tabs):
    ent, ent_aux, rel, rel_aux = tabs
    return ref.proj_chunk_width(ent.shape[1], ent.ctypes.data, 0 if ent_aux is None else ent_aux.ctypes.data, 4,
                                rel.ctypes.data, rel_aux.ctypes.data, 4)


def batch(rng, b, k, ent_rows, rel_rows):
    src, dst = rng.integers(0, ent_rows, b), rng.integers(0, ent_rows, b)
    rel_id = rng.integers(0, rel_rows, b)
    neg = rng.integers(0, ent_rows, (b, k)) if k else None
    return src, rel_id, dst, neg


def run(L, proj, tabs, src, rel_id, dst, neg, kind, corrupt, v=0, g_pos=None, g_neg=None):
    """the host build: forward -> (pos, neg_out); with g_pos the gradient -> the eight row blocks
    (the entity aux blocks None for hyperplane)"""
    ent, ent_aux, rel, rel_aux = tabs
    b, d = len(src), ent.shape[1]
    k = 0 if neg is None else neg.shape[1]
    kp = 2 * k if corrupt == "both" else k
    src, rel_id, dst = (np.ascontiguousarray(x, np.int64) for x in (src, rel_id, dst))
    neg = None if neg is None else np.ascontiguousarray(neg, np.int64)
    head = (ref.PROJ[proj], ref.KIND[kind], ref.CORRUPT[corrupt], v, fp(ent), fp(ent_aux), ent.shape[0], fp(rel),
            fp(rel_aux), rel.shape[0], ip(src), ip(rel_id), ip(dst), ip(neg), b, k, d)
    if g_pos is None:
        pos, out = np.full(b, np.nan, np.float32), np.full((b, kp), np.nan, np.float32)
        assert L.kg_proj_triple(*head, fp(pos), fp(out), *([None] * 10)) == 0
        return pos, out
    g_pos = np.ascontiguousarray(g_pos, np.float32)
    g_neg = None if g_neg is None else np.ascontiguousarray(g_neg, np.float32)
    flat = lambda: np.full((b, d), np.nan, np.float32)                                  # noqa: E731
    block = lambda: np.full((b, k, d), np.nan, np.float32)                              # noqa: E731
    gs, gr, gd, gn, gra = flat(), flat(), flat(), block(), flat()
    gsa, gda, gna = (flat(), flat(), block()) if proj == "transfer" else (None, None, None)
    assert L.kg_proj_triple(*head, None, None, fp(g_pos), fp(g_neg), fp(gs), fp(gr), fp(gd), fp(gn), fp(gra),
                            fp(gsa), fp(gda), fp(gna)) == 0
    return gs, gr, gd, gn, gra, gsa, gda, gna


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_both(L, proj, tabs, src, rel_id, dst, neg, kind, corrupt, rng, v=0):
    """forward and gradient bits of the host build == the restatement; -> the gradient rows"""
    b = len(src)
    k = 0 if neg is None else neg.shape[1]
    kp = 2 * k if corrupt == "both" else k
    vv = v or width(tabs)
    assert v or vv == L.kg_proj_chunk_width(tabs[0].shape[1], fp(tabs[0]), fp(tabs[1]), fp(tabs[2]), fp(tabs[3]))
    tag = (proj, kind, corrupt, k, vv)
    pos, out = run(L, proj, tabs, src, rel_id, dst, neg, kind, corrupt, v)
    want_pos, want_out = ref.forward(proj, *tabs, src, rel_id, dst, neg, kind, corrupt, vv)
    assert same(pos, want_pos) and same(out, want_out), tag
    g_pos = (rng.random(b) * 2 - 1).astype(np.float32)
    g_neg = (rng.random((b, kp)) * 2 - 1).astype(np.float32) if k else None
    got = run(L, proj, tabs, src, rel_id, dst, neg, kind, corrupt, v, g_pos, g_neg)
    want = ref.grad(proj, *tabs, src, rel_id, dst, neg, kind, corrupt, vv, g_pos, g_neg)
    for g, w, name in zip(got, want, NAMES):
        assert same(g, w), tag + (name,)
    return got


@pytest.mark.parametrize("d", ref.DIMS)
def test_host_build_equals_the_restatement(KG, d):
    """V = 1 / 4 / 8 by d, one and several chunks a lane, every butterfly width; 2 projections x
    2 kinds x 3 corrupt modes x K in {0, 1, 5}; B = 11, 40 entity rows, 5 relation rows"""
    rng = np.random.default_rng(100 + d)
    t = Tables(rng, d)
    for k in (0, 1, 5):
        src, rel_id, dst, neg = batch(rng, 11, k, 40, 5)
        for proj in PROJS:
            for kind in KINDS:
                for corrupt in (CORRUPTS if k else ("both",)):
                    check_both(KG, proj, t.of(proj), src, rel_id, dst, neg, kind, corrupt, rng)


@pytest.mark.parametrize("d", [8, 64, 520])
def test_unaligned_table_start_and_forced_widths(KG, d):
    """tables one element past a 16-byte boundary take V = 1 - one such table among aligned ones
    is enough; V in {1, 4, 8} forced"""
    rng = np.random.default_rng(7 + d)
    t, t0 = Tables(rng, d, shift=1), Tables(rng, d)
    src, rel_id, dst, neg = batch(rng, 9, 5, 40, 5)
    for proj in PROJS:
        tabs = t.of(proj)
        assert width(tabs) == 1 == KG.kg_proj_chunk_width(d, *(fp(x) for x in tabs))
        assert width(t0.of(proj)) == 8
        mixed = list(t0.of(proj))
        mixed[3] = tabs[3]                                        # only the relation aux table is off
        assert width(mixed) == 1 == KG.kg_proj_chunk_width(d, *(fp(x) for x in mixed))
        if proj == "transfer":
            mixed = list(t0.of(proj))
            mixed[1] = tabs[1]                                    # only ent_transfer is off
            assert width(mixed) == 1 == KG.kg_proj_chunk_width(d, *(fp(x) for x in mixed))
        for kind in KINDS:
            check_both(KG, proj, tabs, src, rel_id, dst, neg, kind, "both", rng)
            check_both(KG, proj, mixed, src, rel_id, dst, neg, kind, "both", rng)
            for v in (1, 4, 8):
                check_both(KG, proj, tabs, src, rel_id, dst, neg, kind, "both", rng, v=v)
    # 16-bit tables: 8-byte starts give V = 4, all four tables count
    assert ref.proj_chunk_width(d, 16, 32, 2, 48, 64, 2) == 8 and ref.proj_chunk_width(d, 16, 8, 2, 48, 64, 2) == 4
    assert ref.proj_chunk_width(d, 16, 0, 2, 48, 8, 4) == 1 and ref.proj_chunk_width(d, 16, 0, 2, 48, 2, 2) == 1


@pytest.mark.parametrize("proj", PROJS)
@pytest.mark.parametrize("kind", KINDS)
def test_ids_that_name_no_row(KG, proj, kind):
    """-1, rows + 3 and 2^33 + 5 in every id column: never read, rows of zeros in every table the
    id indexes, zero gradient rows; the scores of tables with a zero row appended"""
    rng = np.random.default_rng(11)
    d, ent_rows, rel_rows = 20, 40, 5
    t = Tables(rng, d)
    tabs = t.of(proj)
    bad_e, bad_r = [-1, ent_rows + 3, (1 << 33) + 5], [-1, rel_rows + 3, (1 << 33) + 5]
    src, rel_id, dst, neg = batch(rng, 12, 5, ent_rows, rel_rows)
    src[0:3], dst[3:6], rel_id[6:9] = bad_e, bad_e, bad_r
    neg[9, 0:3] = bad_e
    neg[0, 4] = -1                                            # beside a bad src
    gs, gr, gd, gn, gra, gsa, gda, gna = check_both(KG, proj, tabs, src, rel_id, dst, neg, kind, "both", rng)
    zero = np.zeros(d, np.float32)
    assert all(same(gs[i], zero) for i in range(3)) and all(same(gd[i], zero) for i in range(3, 6))
    assert all(same(gr[i], zero) and same(gra[i], zero) for i in range(6, 9))
    assert all(same(gn[9, j], zero) for j in range(3)) and same(gn[0, 4], zero)
    assert gs[3:].any() and gn[9, 3:].any() and gra[:6].any()
    if proj == "transfer":
        assert all(same(gsa[i], zero) for i in range(3)) and all(same(gda[i], zero) for i in range(3, 6))
        assert all(same(gna[9, j], zero) for j in range(3)) and same(gna[0, 4], zero) and gsa[3:].any()
    # a bad id is a row of zeros: the same scores as tables with a zero row at that id
    pad = lambda x: None if x is None else placed(np.concatenate([x, np.zeros((1, d), np.float32)]))   # noqa: E731
    fix = lambda ids: np.where((ids >= 0) & (ids < ent_rows), ids, ent_rows)                            # noqa: E731
    rfix = np.where((rel_id >= 0) & (rel_id < rel_rows), rel_id, rel_rows)
    pos, out = run(KG, proj, tabs, src, rel_id, dst, neg, kind, "both")
    pos0, out0 = run(KG, proj, [pad(x) for x in tabs], fix(src), rfix, fix(dst), fix(neg), kind, "both")
    assert same(pos, pos0) and same(out, out0)


@pytest.mark.parametrize("kind", KINDS)
def test_all_zero_hyper_and_rel_transfer_rows(KG, kind):
    """hyperplane: w = 0 projects nothing and hyper's row takes gx = inv * gw (ss under the clamp);
    transfer: rho = 0 gives z = x"""
    rng = np.random.default_rng(12)
    t = Tables(rng, 8)
    t.hyper[1] = 0
    t.rel_transfer[1] = 0
    t.rel[2] = 0
    src, rel_id, dst = np.array([3, 0, 4, 3]), np.array([1, 1, 2, 0]), np.array([1, 3, 3, 4])
    neg = np.array([[3, 5], [4, 3], [6, 3], [3, 4]])
    for proj in PROJS:
        got = check_both(KG, proj, t.of(proj), src, rel_id, dst, neg, kind, "both", rng)
        assert all(np.isfinite(g).all() for g in got if g is not None) and got[0][0].any()
        pos, out = run(KG, proj, t.of(proj), src, rel_id, dst, neg, kind, "both")
        assert np.isfinite(pos).all() and np.isfinite(out).all()
        if proj == "transfer":                                  # rho = 0: ent_transfer gets q * x = 0
            assert not got[5][0].any() and not got[5][1].any() and got[5][3].any()


@pytest.mark.parametrize("kind", KINDS)
def test_transfer_row_with_z_zero(KG, kind):
    """an all-zero entity row (z = 0) and one of 1e-8 (ss = 8e-16): TransD's ss under the clamp,
    inv = 1 / sqrt(1e-12f), gz = inv * gy; everything finite"""
    rng = np.random.default_rng(16)
    t = Tables(rng, 8)
    t.ent[3] = 0
    t.ent[4] = np.float32(1e-8)
    src, rel_id, dst = np.array([3, 0, 4, 3]), np.array([0, 1, 2, 1]), np.array([1, 3, 3, 4])
    neg = np.array([[3, 5], [4, 3], [6, 3], [3, 4]])
    for proj in PROJS:
        got = check_both(KG, proj, t.of(proj), src, rel_id, dst, neg, kind, "both", rng)
        assert all(np.isfinite(g).all() for g in got if g is not None) and got[0][0].any()
        pos, out = run(KG, proj, t.of(proj), src, rel_id, dst, neg, kind, "both")
        assert np.isfinite(pos).all() and np.isfinite(out).all()


@pytest.mark.parametrize("proj", PROJS)
def test_zero_l2_norm_has_zero_gradients(KG, proj):
    """src == dst and r a zero row, trans_l2: q == 0 and every gradient of the triple is 0, not NaN"""
    rng = np.random.default_rng(14)
    d = 20
    t = Tables(rng, d)
    t.rel[2] = 0
    src, rel_id, dst, neg = np.array([7, 7]), np.array([2, 2]), np.array([7, 8]), np.array([[7], [9]])
    pos, out = run(KG, proj, t.of(proj), src, rel_id, dst, neg, "trans_l2", "both")
    assert pos[0] == 0 and out[0, 0] == 0 and out[0, 1] == 0 and pos[1] != 0
    got = check_both(KG, proj, t.of(proj), src, rel_id, dst, neg, "trans_l2", "both", rng)
    assert all(not g[0].any() for g in got if g is not None)
    assert all(np.isfinite(g).all() for g in got if g is not None) and got[0][1].any()


@pytest.mark.parametrize("proj", PROJS)
@pytest.mark.parametrize("kind", KINDS)
def test_negative_equal_to_src(KG, proj, kind):
    """n == src: the tail score is s(h, r, h); its rows get separate gradient rows, which the
    table's gradient accumulates in occurrence order"""
    rng = np.random.default_rng(15)
    t = Tables(rng, 64)
    src, rel_id, dst = np.array([4, 9, 4]), np.array([0, 1, 1]), np.array([5, 9, 6])
    neg = np.array([[4, 4, 7], [9, 1, 9], [6, 4, 5]])
    got = check_both(KG, proj, t.of(proj), src, rel_id, dst, neg, kind, "both", rng)
    gs, gd, gn = got[0], got[2], got[3]
    assert gn[0, 0].any() and gs[0].any()
    keys = np.concatenate([src, dst, neg.reshape(-1)])
    table = ref.scatter_rows(np.concatenate([gs, gd, gn.reshape(-1, 64)]), keys, 40)
    assert same(table[4], ((gs[0] + gs[2]) + gn[0, 0] + gn[0, 1]) + gn[2, 1])


# ---- float64: the restatement against the torch autograd composition --------------------------
def composition64(torch, proj, tabs, src, rel_id, dst, neg, kind, corrupt):
    """generate_embedding and calculate_scores as the reference spells them (transH.py:43-66,
    transD.py:46-73, transX.py:105-133), in torch float64: lookups, the tile of the relation's
    rows over the negatives, projection, tf.nn.l2_normalize, the scores, the concat"""
    ent, ent_aux, rel, rel_aux = tabs
    eps = float(np.float32(1e-12))
    k = neg.shape[1]

    def l2n(x):
        return x * torch.rsqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=eps))

    def project(x, ids, aux):
        if proj == "hyperplane":
            w = l2n(aux)
            return x - (x * w).sum(-1, keepdim=True) * w
        return l2n(x + (x * ent_aux[ids]).sum(-1, keepdim=True) * aux)

    def score(a, r, c):
        e = a + r - c
        return -(e.abs().sum(-1) if kind == "trans_l1" else torch.sqrt((e * e).sum(-1)))

    aux = rel_aux[rel_id].unsqueeze(1)                            # [B, 1, d]
    aux_k = aux.repeat(1, k, 1)                                   # the tile over the negatives
    h = project(ent[src].unsqueeze(1), src.unsqueeze(1), aux)
    t = project(ent[dst].unsqueeze(1), dst.unsqueeze(1), aux)
    n = project(ent[neg], neg, aux_k)
    r = l2n(rel[rel_id].unsqueeze(1))
    hh, rr, tt = h.repeat(1, k, 1), r.repeat(1, k, 1), t.repeat(1, k, 1)
    front, tail = score(n, rr, tt), score(hh, rr, n)
    out = front if corrupt == "front" else tail if corrupt == "tail" else torch.cat([front, tail], 1)
    return score(h, r, t).reshape(-1), out


def close64(a, b):
    """the project's criterion for two float64 forms (tests/test_triple_score_gpu.py)"""
    return np.all(np.abs(a - b) <= 1e-9 * (1 + np.abs(b)))


@pytest.mark.parametrize("proj", PROJS)
@pytest.mark.parametrize("kind", KINDS)
def test_float64_restatement_equals_the_torch_autograd_composition(proj, kind):
    """forward and the gradients of every table; random rows, src != dst and no id out of range, so
    no trans_l1 residual is exactly 0 and no trans_l2 norm is 0"""
    import torch
    for d, corrupt in ((3, "both"), (20, "front"), (64, "tail")):
        rng = np.random.default_rng(500 + d)
        t = Tables(rng, d, wide=False)
        tabs = t.of(proj)
        b, k = 11, 5
        src, rel_id, _, neg = batch(rng, b, k, 40, 5)
        dst = (src + 1 + rng.integers(0, 38, b)) % 40
        kp = 2 * k if corrupt == "both" else k
        g_pos, g_neg = rng.random(b) * 2 - 1, rng.random((b, kp)) * 2 - 1
        pos, out = ref.forward(proj, *tabs, src, rel_id, dst, neg, kind, corrupt, 1, dt=np.float64)
        rows = ref.grad(proj, *tabs, src, rel_id, dst, neg, kind, corrupt, 1, g_pos, g_neg, dt=np.float64)
        tt = [None if x is None else torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in tabs]
        ids = [torch.from_numpy(np.asarray(x, np.int64)) for x in (src, rel_id, dst, neg)]
        p64, o64 = composition64(torch, proj, tt, *ids, kind, corrupt)
        assert close64(pos, p64.detach().numpy()) and close64(out, o64.detach().numpy()), (d, "forward")
        ((p64 * torch.from_numpy(g_pos)).sum() + (o64 * torch.from_numpy(g_neg)).sum()).backward()
        keys = np.concatenate([src, dst, neg.reshape(-1)])
        gs, gr, gd, gn, gra, gsa, gda, gna = rows
        want = {0: ref.scatter_rows(np.concatenate([gs, gd, gn.reshape(-1, d)]), keys, 40),
                2: ref.scatter_rows(gr, rel_id, 5), 3: ref.scatter_rows(gra, rel_id, 5)}
        if proj == "transfer":
            want[1] = ref.scatter_rows(np.concatenate([gsa, gda, gna.reshape(-1, d)]), keys, 40)
        for i, table in want.items():
            assert table.any() and close64(table, tt[i].grad.numpy()), (d, "table", i)


# ---- the fp32 restatement within the derived bound of float64 ---------------------------------
@pytest.mark.parametrize("proj", PROJS)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_within_the_derived_bound_of_float64(proj, kind, capsys):
    """|fp32 restatement - float64| <= gamma(n(proj, kind, d)) * (the float64 sum of the magnitudes
    of the terms), no margin; rows uniform in [-4, 4], transfer rows in [-1, 1]"""
    worst = 0.0
    for d in ref.DIMS:
        rng = np.random.default_rng(1000 + d)
        t = Tables(rng, d, ent_rows=300, rel_rows=7, wide=False)
        tabs = t.of(proj)
        src, rel_id, dst, neg = batch(rng, 90, 5, 300, 7)
        for v in {1, width(tabs)}:
            pos, out = ref.forward(proj, *tabs, src, rel_id, dst, neg, kind, "both", v)
            p64, o64, mp, mo = ref.forward64(proj, *tabs, src, rel_id, dst, neg, kind, "both")
            for got, want, mag in ((pos, p64, mp), (out, o64, mo)):
                err, bound = np.abs(got.astype(np.float64) - want), ref.forward_bound(proj, kind, d, mag)
                known = np.isfinite(bound)
                assert known.mean() > 0.9 and np.all(err[known] <= bound[known]), \
                    (d, v, float((err[known] / bound[known]).max()))
                worst = max(worst, float((err[known] / np.maximum(bound[known], 1e-300)).max()))
    with capsys.disabled():
        print("\n[triple_score_proj %s %s] worst error / bound = %.4f" % (proj, kind, worst))
    assert 0 < worst <= 1


# ---- plumbing ---------------------------------------------------------------------------------
def test_new_entries_are_exported_and_bound():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    for name, n_args in (("euler_gpu_triple_score_proj", 21), ("euler_gpu_triple_score_proj_grad", 29)):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
        assert name + "(" in hdr
        assert len(_lib.SIGNATURES[name][1]) == n_args


def test_sources_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "$(HERE)kg_proj.h" in mk and "kg_proj_kernels.hip" in mk


def test_op_is_public():
    from euler_amd import ops
    assert callable(ops.triple_score_proj)
