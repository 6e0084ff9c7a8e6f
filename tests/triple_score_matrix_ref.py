"""The numpy restatement of euler_amd/csrc/kg_matrix.h (triple scoring with TransR's per-relation
matrix projection fused in): elementwise operations in the stated orders, forward, per-occurrence
gradients and the ordered matrix gradient, vectorised across triples.  It is written over a dtype
as triple_score_proj_ref is: with float32 every ufunc is one correctly rounded operation, every
sum over the dr columns is triple_score_ref.lane_sum and the projection sums run term by term in
the stated order, so these loops and the header return the same bits; with float64 the same
expressions serve as the high-precision form that the torch float64 autograd composition is held
against.

ERROR BOUND of the fp32 forward against float64 (u = 2^-24, gamma(n) = n u / (1 - n u), the model
and the lemma of triple_score_ref; no row's ss near the 1e-12 clamp), derived as
triple_score_proj_ref derives TransD's, with the de-term projection sum in place of its axpy.
  z^_j = sum_c fl(x_c M_cj): de products, each rounded once, and de - 1 additions in any order:
  |z^_j - z_j| <= gamma(de) Z_j, Z_j = sum_c |x_c| |M_cj| >= |z_j|.  The normalisation sees an
  ABSOLUTE perturbation zeta of z, ||zeta|| <= gamma(de) ||Z|| = gamma(de) kappa ||z||,
  kappa = ||Z|| / ||z|| >= 1 (how much the projection cancelled): ||z'|| >= ||z|| (1 - gamma(de)
  kappa) and, with y' = z' / ||z'||, |y'_j - y_j| <= |zeta_j| / ||z'|| + |z_j| ||zeta|| / (||z||
  ||z'||) <= gamma(de) Y_j, Y_j = (Z_j / ||z|| + kappa |y_j|) / (1 - gamma(de) kappa) >= |y_j|;
  no bound exists where gamma(de) kappa >= 1.  The normalisation itself over dr columns:
  y^ = y' (1 + theta_{dr+3}): |y^_j - y_j| <= (gamma(de) (1 + gamma(dr+3)) + gamma(dr+3)) Y_j
  <= gamma(de+dr+3) Y_j.  Residual e = (h + r) - t: h takes two more roundings, t one,
  r^ = r (1 + theta_{dr+5}): |e^ - e| <= gamma(de+dr+5) M, M = Y_h + |r| + Y_t.
  trans_l1: gamma(de+dr+5) + gamma(dr-1) + their product <= gamma(de+2dr+4) on sum M.
  trans_l2: |q^ - q| <= gamma(de+dr+5) sum M + gamma(dr+1) (q + gamma(de+dr+5) sum M), q <= sum M:
  <= gamma(de+2dr+6) sum M.
"""
import numpy as np

from triple_score_ref import CORRUPT, EPS, F, KIND, U, chunk_width, gamma, lane_sum, rows_of  # noqa: F401
from triple_score_proj_ref import _Ops, _contrib, _neg_ids, _norm_grad, _score, scatter_rows  # noqa: F401

KINDS = ("trans_l1", "trans_l2")
MAX_DIM = 512
# (de, dr): V = 1 / 4 / 8 by dr, one to eight chunks a lane, every butterfly width, the tile edges
# of the kernels (16 rows of M in the gx and G_M tiles, 64 columns in the G_M tile) and the cap
DIMS = ((1, 1), (1, 8), (8, 1), (3, 5), (8, 8), (32, 32), (64, 33), (33, 64), (100, 100), (130, 70), (17, 65))


def matrix_chunk_width(dr, rel_addr, rel_itemsize):
    """V of the dr-sums: kg_score.h's rule over `rel` alone"""
    return chunk_width(dr, rel_addr, rel_itemsize, rel_addr, rel_itemsize)


def forward_n(kind, de, dr):
    """n of the forward bound gamma(n) * (the float64 sum of the magnitudes of the terms)"""
    return de + 2 * dr + (4 if kind == "trans_l1" else 6)


def forward_bound(kind, de, dr, mag):
    return gamma(forward_n(kind, de, dr)) * mag


def matrices_of(matrix, rel_id, de, dr, dt):
    """-> M [B, de, dr] with zeros where rel_id names no relation"""
    m, _ = rows_of(np.asarray(matrix, F).reshape(matrix.shape[0], de * dr), rel_id)
    return m.reshape(len(rel_id), de, dr).astype(dt)


def project(x, m):
    """z_j = sum_c x_c * M[c, j]: the terms added one by one in increasing c from the first"""
    z = x[:, 0, None] * m[:, 0, :]
    for c in range(1, x.shape[1]):
        z = z + x[:, c, None] * m[:, c, :]
    return z


def back_project(gz, m):
    """gx_c = sum_j gz_j * M[c, j]: increasing j from the first term"""
    gx = gz[:, 0, None] * m[:, :, 0]
    for j in range(1, gz.shape[1]):
        gx = gx + gz[:, j, None] * m[:, :, j]
    return gx


class _Rel(object):
    """r = N(rel[rel_id]) and M = matrix[rel_id]"""

    def __init__(self, o, rel, matrix, rel_id, de):
        self.x, self.ok = o.rows(rel, rel_id)
        self.ss = o.sum(self.x * self.x)
        self.inv = o.inv(self.ss)
        self.y = self.x * self.inv[:, None]
        self.m = matrices_of(matrix, rel_id, de, rel.shape[1], o.dt)


class _Ent(object):
    """a projected entity row: y is what the scores take"""

    def __init__(self, o, ent, ids, rel):
        self.x, self.ok = o.rows(ent, ids)
        self.z = project(self.x, rel.m)
        self.ss = o.sum(self.z * self.z)
        self.inv = o.inv(self.ss)
        self.y = self.z * self.inv[:, None]


def forward(ent, rel, matrix, src, rel_id, dst, neg, kind, corrupt, v, dt=F):
    """widened fp32 tables, matrix [R, de * dr]; neg [B, K] or None -> (pos [B], neg_out [B, K'])"""
    o = _Ops(dt, v)
    b = len(src)
    neg, k = _neg_ids(neg, b)
    r = _Rel(o, rel, matrix, rel_id, ent.shape[1])
    h, t = _Ent(o, ent, src, r), _Ent(o, ent, dst, r)
    pos = _score(o, kind, h, r, t)
    kp = 2 * k if corrupt == "both" else k
    out = np.zeros((b, kp), dt)
    for j in range(k):
        n = _Ent(o, ent, neg[:, j], r)
        if corrupt != "tail":
            out[:, j] = _score(o, kind, n, r, t)
        if corrupt != "front":
            out[:, (k if corrupt == "both" else 0) + j] = _score(o, kind, h, r, n)
    return pos, out


def _through(o, e, r, gy):
    """a projected row with gy complete -> (gz, gx)"""
    gz = _norm_grad(o, e.y, e.ss, e.inv, gy).astype(o.dt)
    gx = back_project(gz, r.m)
    return gz, np.where(e.ok[:, None], gx, o.dt(0)).astype(o.dt)


def grad(ent, rel, matrix, src, rel_id, dst, neg, kind, corrupt, v, g_pos, g_neg, dt=F):
    """-> the per-occurrence rows (G_src [B, de], G_rel [B, dr], G_dst [B, de], G_neg [B, K, de],
    gz_src, gz_dst [B, dr], gz_neg [B, K, dr])"""
    o = _Ops(dt, v)
    b, de, dr = len(src), ent.shape[1], rel.shape[1]
    neg, k = _neg_ids(neg, b)
    r = _Rel(o, rel, matrix, rel_id, de)
    h, t = _Ent(o, ent, src, r), _Ent(o, ent, dst, r)
    zeros = lambda: np.zeros((b, dr), dt)                                                # noqa: E731
    gh, gr, gt = zeros(), zeros(), zeros()
    kk = _contrib(o, kind, g_pos, h, r, t)
    gh, gr, gt = gh + kk, gr + kk, gt + (-kk)
    g_rows, z_rows = np.zeros((b, k, de), dt), np.zeros((b, k, dr), dt)
    g_neg = np.asarray(g_neg, dt).reshape(b, -1) if k else None
    for j in range(k):
        n = _Ent(o, ent, neg[:, j], r)
        gn = zeros()
        if corrupt != "tail":
            kk = _contrib(o, kind, g_neg[:, j], n, r, t)
            gn, gr, gt = gn + kk, gr + kk, gt + (-kk)
        if corrupt != "front":
            kk = _contrib(o, kind, g_neg[:, (k if corrupt == "both" else 0) + j], h, r, n)
            gh, gr, gn = gh + kk, gr + kk, gn + (-kk)
        z_rows[:, j], g_rows[:, j] = _through(o, n, r, gn)
    gz_src, g_src = _through(o, h, r, gh)
    gz_dst, g_dst = _through(o, t, r, gt)
    g_rel = np.where(r.ok[:, None], _norm_grad(o, r.y, r.ss, r.inv, gr), dt(0)).astype(dt)
    return g_src, g_rel, g_dst, g_rows, gz_src, gz_dst, z_rows


def matrix_grad(ent, n_rel, src, rel_id, dst, neg, gz_src, gz_dst, gz_neg, dt=F):
    """G_M [n_rel, de * dr]: per relation the terms fl(x_c * gz_j) of its occurrences, added one by
    one from the first: by increasing triple, within a triple n_0 .. n_{K-1}, h, t; an occurrence
    whose entity id names no row contributes no term"""
    b, de, dr = len(src), ent.shape[1], gz_src.shape[1]
    neg, k = _neg_ids(neg, b)
    out = np.zeros((n_rel, de, dr), dt)
    started = np.zeros(n_rel, bool)
    table = np.asarray(ent, F).astype(dt)
    for t in range(b):
        rho = int(rel_id[t])
        if not 0 <= rho < n_rel:
            continue
        occ = [(int(neg[t, j]), gz_neg[t, j]) for j in range(k)] + [(int(src[t]), gz_src[t]), (int(dst[t]), gz_dst[t])]
        for i, gz in occ:
            if not 0 <= i < ent.shape[0]:
                continue
            term = table[i][:, None] * np.asarray(gz, dt)[None, :]
            out[rho] = out[rho] + term if started[rho] else term
            started[rho] = True
    return out.reshape(n_rel, de * dr)


# ---- float64: the scores with the magnitude sums of their terms (the bound above) -------------
def forward64(ent, rel, matrix, src, rel_id, dst, neg, kind, corrupt):
    """-> (pos, neg_out, mag_pos, mag_neg) in float64; mag is sum M of the derivation (inf where
    the bound does not exist)"""
    dt = np.float64
    o = _Ops(dt, 1)
    b, de = len(src), ent.shape[1]
    neg, k = _neg_ids(neg, b)
    r = _Rel(o, rel, matrix, rel_id, de)

    def ent_row(ids):
        e = _Ent(o, ent, ids, r)
        big_z = project(np.abs(e.x), np.abs(r.m))
        norm = np.sqrt((e.z * e.z).sum(-1, keepdims=True))
        with np.errstate(divide="ignore", invalid="ignore"):
            kappa = np.sqrt((big_z * big_z).sum(-1, keepdims=True)) / norm
            room = 1.0 - gamma(de) * kappa
            y = (big_z / norm + kappa * np.abs(e.y)) / room
        e.mag = np.where(np.isfinite(y) & (room > 0), y, np.inf)
        return e

    def score(a, c):
        return _score(o, kind, a, r, c), (a.mag + np.abs(r.y) + c.mag).sum(-1)

    h, t = ent_row(src), ent_row(dst)
    pos, mag_pos = score(h, t)
    kp = 2 * k if corrupt == "both" else k
    out, mag = np.zeros((b, kp)), np.zeros((b, kp))
    for j in range(k):
        n = ent_row(neg[:, j])
        if corrupt != "tail":
            out[:, j], mag[:, j] = score(n, t)
        if corrupt != "front":
            at = (k if corrupt == "both" else 0) + j
            out[:, at], mag[:, at] = score(h, n)
    return pos, out, mag_pos, mag
