"""The numpy restatement of euler_amd/csrc/kg_proj.h (triple scoring with the TransH "hyperplane"
and the TransD "transfer" projection fused in): elementwise operations in the stated order,
forward and gradient, vectorised across triples.  It is written over a dtype: with float32 every
ufunc is one correctly rounded operation and every sum over columns is triple_score_ref.lane_sum,
so these loops and the header return the same bits; with float64 the same expressions (sums by
numpy) serve as the high-precision form that the torch float64 autograd composition is held
against.  lane_sum, rows_of and chunk_width are triple_score_ref's.

ERROR BOUNDS of the fp32 forward against float64 (u = 2^-24, gamma(n) = n u / (1 - n u), the
model and the lemma of triple_score_ref; no row's ss near the 1e-12 clamp).  A normalised row has
y^ = y (1 + theta_{d+3}).

hyperplane.  w^ = w (1 + theta_{d+3}).  p^ = sum fl(x_c w^_c): one more rounding per product and
  d - 1 additions: |p^ - p| <= gamma(2d+3) P, P = sum |x_c| |w_c|.  m_c = fl(p^ w^_c) =
  p^ w_c (1 + theta_{d+4}): |m^_c - p w_c| <= (gamma(2d+3) (1 + gamma(d+4)) + gamma(d+4)) P |w_c|
  <= gamma(3d+7) P |w_c|.  xp_c = fl(x_c - m^_c): |xp^_c - xp_c| <= gamma(3d+7) P |w_c| +
  u (|x_c| + (1 + gamma(3d+7)) P |w_c|) <= gamma(3d+8) X_c, X_c = |x_c| + P |w_c| >= |xp_c|.
  Residual e = (hp + r) - tp: hp takes two more roundings, tp one, r^ = r (1 + theta_{d+5}):
  |e^ - e| <= gamma(3d+10) M, M = X_h + |r| + X_t.
  trans_l1: gamma(3d+10) + gamma(d-1) + their product <= gamma(4d+9) on sum M.
  trans_l2: |q^ - q| <= gamma(3d+10) sum M + gamma(d+1) (q + gamma(3d+10) sum M), q <= sum M:
  <= gamma(4d+11) sum M.
transfer.  p^ = sum fl(x_c a_c): |p^ - p| <= gamma(d) P, P = sum |x_c| |a_c|.  m_c = fl(p^ rho_c):
  |m^_c - p rho_c| <= gamma(d+1) P |rho_c|.  z_c = fl(x_c + m^_c): |z^_c - z_c| <= gamma(d+2) Z_c,
  Z_c = |x_c| + P |rho_c|.  The normalisation sees an ABSOLUTE perturbation zeta of z,
  ||zeta|| <= gamma(d+2) ||Z|| = gamma(d+2) kappa ||z||, kappa = ||Z|| / ||z|| >= 1 (how much the
  projection cancelled): ||z'|| >= ||z|| (1 - gamma(d+2) kappa) and, with y' = z' / ||z'||,
  |y'_c - y_c| <= |zeta_c| / ||z'|| + |z_c| ||zeta|| / (||z|| ||z'||) <= gamma(d+2) Y_c,
  Y_c = (Z_c / ||z|| + kappa |y_c|) / (1 - gamma(d+2) kappa) >= |y_c|: the magnitude of a
  projected column carries kappa, and no bound exists where gamma(d+2) kappa >= 1.  The
  normalisation itself: y^ = y' (1 + theta_{d+3}): |y^_c - y_c| <= (gamma(d+2) (1 + gamma(d+3)) +
  gamma(d+3)) Y_c <= gamma(2d+5) Y_c.  Residual: |e^ - e| <= gamma(2d+7) M, M = Y_h + |r| + Y_t.
  trans_l1: gamma(2d+7) + gamma(d-1) + their product <= gamma(3d+6) on sum M.
  trans_l2: as above with gamma(d+1): <= gamma(3d+8) sum M.
"""
import numpy as np

from triple_score_ref import CORRUPT, DIMS, EPS, F, KIND, U, chunk_width, gamma, lane_sum, rows_of  # noqa: F401

PROJ = {"hyperplane": 1, "transfer": 2}
KINDS = ("trans_l1", "trans_l2")


def proj_chunk_width(d, ent_addr, ent_aux_addr, ent_itemsize, rel_addr, rel_aux_addr, rel_itemsize):
    """V over every table passed (an absent table: address 0)"""
    return min(chunk_width(d, ent_addr, ent_itemsize, rel_addr, rel_itemsize),
               chunk_width(d, ent_aux_addr, ent_itemsize, rel_aux_addr, rel_itemsize))


def forward_n(proj, kind, d):
    """n of the forward bound gamma(n) * (the float64 sum of the magnitudes of the terms)"""
    return {("hyperplane", "trans_l1"): 4 * d + 9, ("hyperplane", "trans_l2"): 4 * d + 11,
            ("transfer", "trans_l1"): 3 * d + 6, ("transfer", "trans_l2"): 3 * d + 8}[proj, kind]


def forward_bound(proj, kind, d, mag):
    return gamma(forward_n(proj, kind, d)) * mag


class _Ops(object):
    """the dtype and the sum over columns"""

    def __init__(self, dt, v):
        self.dt, self.v, self.eps = dt, v, dt(EPS)

    def sum(self, terms):
        return lane_sum(terms, self.v) if self.dt is F else terms.sum(-1)

    def rows(self, table, ids):
        x, ok = rows_of(table, ids)
        return x.astype(self.dt), ok

    def inv(self, ss):
        return self.dt(1) / np.sqrt(np.where(ss > self.eps, ss, self.eps))


class _Rel(object):
    """r = N(rel[rel_id]) and the aux row: w = N(hyper[rel_id]) or rho = rel_transfer[rel_id]"""

    def __init__(self, o, proj, rel, rel_aux, rel_id):
        self.x, self.ok = o.rows(rel, rel_id)
        self.ss = o.sum(self.x * self.x)
        self.inv = o.inv(self.ss)
        self.y = self.x * self.inv[:, None]
        self.aux, _ = o.rows(rel_aux, rel_id)
        if proj == "hyperplane":
            self.aux_ss = o.sum(self.aux * self.aux)
            self.aux_inv = o.inv(self.aux_ss)
            self.w = self.aux * self.aux_inv[:, None]
        else:
            self.w = self.aux * o.dt(1)


class _Ent(object):
    """a projected entity row: y is what the scores take"""

    def __init__(self, o, proj, ent, ent_aux, ids, rel):
        self.x, self.ok = o.rows(ent, ids)
        if proj == "hyperplane":
            self.p = o.sum(self.x * rel.w)
            self.y = self.x + (-(self.p[:, None] * rel.w))
        else:
            self.a, _ = o.rows(ent_aux, ids)
            self.p = o.sum(self.x * self.a)
            self.z = self.x + self.p[:, None] * rel.w
            self.ss = o.sum(self.z * self.z)
            self.inv = o.inv(self.ss)
            self.y = self.z * self.inv[:, None]


def _score(o, kind, a, r, c):
    e = (a.y + r.y) - c.y
    s = o.sum(np.abs(e) if kind == "trans_l1" else e * e)
    return -s if kind == "trans_l1" else -np.sqrt(s)


def _neg_ids(neg, b):
    if neg is None:
        return None, 0
    neg = np.asarray(neg).reshape(b, -1)
    return neg, neg.shape[1]


def forward(proj, ent, ent_aux, rel, rel_aux, src, rel_id, dst, neg, kind, corrupt, v, dt=F):
    """widened fp32 tables (ent_aux None for hyperplane); neg [B, K] or None -> (pos [B], neg_out [B, K'])"""
    o = _Ops(dt, v)
    b = len(src)
    neg, k = _neg_ids(neg, b)
    r = _Rel(o, proj, rel, rel_aux, rel_id)
    h, t = _Ent(o, proj, ent, ent_aux, src, r), _Ent(o, proj, ent, ent_aux, dst, r)
    pos = _score(o, kind, h, r, t)
    kp = 2 * k if corrupt == "both" else k
    out = np.zeros((b, kp), dt)
    for j in range(k):
        n = _Ent(o, proj, ent, ent_aux, neg[:, j], r)
        if corrupt != "tail":
            out[:, j] = _score(o, kind, n, r, t)
        if corrupt != "front":
            out[:, (k if corrupt == "both" else 0) + j] = _score(o, kind, h, r, n)
    return pos, out


def _contrib(o, kind, g, a, r, c):
    """what one scored triple adds to gy_a and gy_r (kk) and to gy_c (-kk)"""
    g = np.asarray(g, o.dt)
    e = (a.y + r.y) - c.y
    if kind == "trans_l1":
        gg = np.broadcast_to(g[:, None], e.shape)
        return np.where(e > 0, -gg, np.where(e < 0, gg, o.dt(0))).astype(o.dt)
    q = np.sqrt(o.sum(e * e))
    with np.errstate(divide="ignore", invalid="ignore"):
        gq = np.where(q == 0, o.dt(0), g / q).astype(o.dt)
    return -(gq[:, None] * e)


def _norm_grad(o, y, ss, inv, gy):
    dot = o.sum(y * gy)[:, None]
    inv = inv[:, None]
    return np.where((ss > o.eps)[:, None], inv * (gy + (-(y * dot))), inv * gy)


def _through(o, proj, e, r, gy, gaux):
    """an entity row with gy complete -> (gx, ga | None, gaux with the row's term)"""
    ok, zero = e.ok[:, None], o.dt(0)
    if proj == "hyperplane":
        q = o.sum(gy * r.w)[:, None]
        gx = gy + (-(q * r.w))
        gaux = gaux + (-((q * e.x) + (e.p[:, None] * gy)))
        return np.where(ok, gx, zero).astype(o.dt), None, gaux
    gz = _norm_grad(o, e.y, e.ss, e.inv, gy)
    q = o.sum(gz * r.w)[:, None]
    gx, ga = gz + q * e.a, q * e.x
    gaux = gaux + e.p[:, None] * gz
    return np.where(ok, gx, zero).astype(o.dt), np.where(ok, ga, zero).astype(o.dt), gaux


def grad(proj, ent, ent_aux, rel, rel_aux, src, rel_id, dst, neg, kind, corrupt, v, g_pos, g_neg, dt=F):
    """-> the per-occurrence gradients of the raw rows: (G_src, G_rel, G_dst [B, d], G_neg [B, K, d],
    G_rel_aux [B, d], G_src_aux, G_dst_aux [B, d], G_neg_aux [B, K, d]); the last three None for
    hyperplane"""
    o = _Ops(dt, v)
    b, d = len(src), ent.shape[1]
    neg, k = _neg_ids(neg, b)
    r = _Rel(o, proj, rel, rel_aux, rel_id)
    h, t = _Ent(o, proj, ent, ent_aux, src, r), _Ent(o, proj, ent, ent_aux, dst, r)
    zeros = lambda: np.zeros((b, d), dt)                                                 # noqa: E731
    gh, gr, gt, gaux = zeros(), zeros(), zeros(), zeros()
    kk = _contrib(o, kind, g_pos, h, r, t)
    gh, gr, gt = gh + kk, gr + kk, gt + (-kk)
    g_rows, a_rows = np.zeros((b, k, d), dt), np.zeros((b, k, d), dt)
    g_neg = np.asarray(g_neg, dt).reshape(b, -1) if k else None
    for j in range(k):
        n = _Ent(o, proj, ent, ent_aux, neg[:, j], r)
        gn = zeros()
        if corrupt != "tail":
            kk = _contrib(o, kind, g_neg[:, j], n, r, t)
            gn, gr, gt = gn + kk, gr + kk, gt + (-kk)
        if corrupt != "front":
            kk = _contrib(o, kind, g_neg[:, (k if corrupt == "both" else 0) + j], h, r, n)
            gh, gr, gn = gh + kk, gr + kk, gn + (-kk)
        g_rows[:, j], ga, gaux = _through(o, proj, n, r, gn, gaux)
        if ga is not None:
            a_rows[:, j] = ga
    g_src, g_src_aux, gaux = _through(o, proj, h, r, gh, gaux)
    g_dst, g_dst_aux, gaux = _through(o, proj, t, r, gt, gaux)
    rok, zero = r.ok[:, None], dt(0)
    g_rel = np.where(rok, _norm_grad(o, r.y, r.ss, r.inv, gr), zero).astype(dt)
    if proj == "hyperplane":
        g_rel_aux = np.where(rok, _norm_grad(o, r.w, r.aux_ss, r.aux_inv, gaux), zero).astype(dt)
        return g_src, g_rel, g_dst, g_rows, g_rel_aux, None, None, None
    g_rel_aux = np.where(rok, gaux, zero).astype(dt)
    return g_src, g_rel, g_dst, g_rows, g_rel_aux, g_src_aux, g_dst_aux, a_rows


# ---- float64: the scores with the magnitude sums of their terms (the bounds above) ------------
def forward64(proj, ent, ent_aux, rel, rel_aux, src, rel_id, dst, neg, kind, corrupt):
    """-> (pos, neg_out, mag_pos, mag_neg) in float64; mag is sum M of the derivation (inf where
    the transfer bound does not exist)"""
    dt = np.float64
    o = _Ops(dt, 1)
    b, d = len(src), ent.shape[1]
    neg, k = _neg_ids(neg, b)
    r = _Rel(o, proj, rel, rel_aux, rel_id)

    def mags(e):
        if proj == "hyperplane":
            big_p = (np.abs(e.x) * np.abs(r.w)).sum(-1, keepdims=True)
            return np.abs(e.x) + big_p * np.abs(r.w)
        big_p = (np.abs(e.x) * np.abs(e.a)).sum(-1, keepdims=True)
        big_z = np.abs(e.x) + big_p * np.abs(r.w)
        norm = np.sqrt((e.z * e.z).sum(-1, keepdims=True))
        with np.errstate(divide="ignore", invalid="ignore"):
            kappa = np.sqrt((big_z * big_z).sum(-1, keepdims=True)) / norm
            room = 1.0 - gamma(d + 2) * kappa
            y = (big_z / norm + kappa * np.abs(e.y)) / room
        return np.where(np.isfinite(y) & (room > 0), y, np.inf)

    def ent_row(ids):
        e = _Ent(o, proj, ent, ent_aux, ids, r)
        e.mag = mags(e)
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


def scatter_rows(rows, keys, size):
    """scatter_add in input order; keys outside [0, size) drop out"""
    out = np.zeros((size, rows.shape[1]), rows.dtype)
    for p, key in enumerate(np.asarray(keys, np.int64)):
        if 0 <= key < size:
            out[key] = out[key] + rows[p]
    return out
