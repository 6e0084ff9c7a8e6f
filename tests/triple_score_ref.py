"""The numpy restatement of euler_amd/csrc/kg_score.h (fused triple scoring for TransE l1 / l2 and
DistMult): fp32 operations in the stated order, forward and gradient, vectorised across triples;
a float64 formulation of the reference's TensorFlow expressions (calculate_energy of
examples/TransX/transX.py and examples/distmult/distmult.py); and the error bounds derived below.

Every numpy float32 ufunc used here (+, -, *, /, sqrt, abs, comparisons) is one correctly
rounded operation, so these loops and the header return the same bits.

ERROR BOUNDS (u = 2^-24, gamma(n) = n u / (1 - n u), no underflow; Higham, Accuracy and
Stability of Numerical Algorithms, Lemma 3.1: a product of n factors (1 + delta_i)^(+-1),
|delta_i| <= u, is 1 + theta_n with |theta_n| <= gamma(n), and gamma(j) + gamma(k) +
gamma(j) gamma(k) <= gamma(j + k)).  A sum of d terms in ANY order passes every term through at
most d - 1 additions.

Normalised row: ss^ = ss (1 + theta_d) (one product, d - 1 adds; all terms >= 0); the clamp is
1-Lipschitz; the square root halves the relative error (<= theta_d) and rounds once, the
reciprocal rounds once: inv^ = inv (1 + theta_{d+2}), y^ = y (1 + theta_{d+3}).  Without
normalize y^ = y, which the same bounds cover.
Residual e = (a + r) - c: e^ = e + eta, |eta| <= gamma(d+5) M, M = |a| + |r| + |c| (a and r
take two more roundings, c one).
trans_l1: | |e^| - |e| | <= |eta|; the sum adds theta_{d-1} on sum |e^| <= (1 + gamma(d+5)) sum M:
   |s^ - s| <= (gamma(d+5) + gamma(d-1) + gamma(d+5) gamma(d-1)) sum M <= gamma(2d+4) sum M.
trans_l2: q' = ||e^||_2 has |q' - q| <= ||eta||_2 <= ||eta||_1 <= gamma(d+5) sum M; the sum of
   squares is (1 + theta_d) (one product, d - 1 adds), its root (1 + theta_{d+1}):
   |q^ - q| <= gamma(d+5) sum M + gamma(d+1) (q + gamma(d+5) sum M), q <= sum M:
   |s^ - s| <= gamma(2d+6) sum M.
distmult: each factor is (1 + theta_{d+3}), two products, d - 1 adds:
   |s^ - s| <= gamma(4d+10) sum |a r c|.
"""
import numpy as np

F = np.float32
KIND = {"trans_l1": 0, "trans_l2": 1, "distmult": 2}
CORRUPT = {"front": 0, "tail": 1, "both": 2}
EPS = F(1e-12)
U = 2.0 ** -24
DIMS = (1, 3, 8, 20, 64, 128, 200, 256, 512, 520)        # tests/test_half_mp_gpu.py


def gamma(n):
    return n * U / (1.0 - n * U)


def forward_n(kind, d):
    """n of the forward bound gamma(n) * (the float64 sum of the magnitudes of the terms)"""
    return {"trans_l1": 2 * d + 4, "trans_l2": 2 * d + 6, "distmult": 4 * d + 10}[kind]


def chunk_width(d, ent_addr, ent_itemsize, rel_addr, rel_itemsize):
    """V of the stated order, from d and the addresses (or their low bits) of the two tables"""
    a16 = ent_addr % 16 == 0 and rel_addr % 16 == 0
    a4 = ent_addr % (16 if ent_itemsize == 4 else 8) == 0 and rel_addr % (16 if rel_itemsize == 4 else 8) == 0
    return 8 if d % 8 == 0 and a16 else 4 if d % 4 == 0 and a4 else 1


def lanes_of(chunks):
    lanes = 1
    while lanes < 64 and lanes < chunks:
        lanes *= 2
    return lanes


def lane_sum(terms, v):
    """[N, d] fp32 terms -> [N] sums in the stated order: lane l adds the terms of the chunks
    l, l + L, ... one by one from its first term, then the xor butterfly"""
    terms = np.ascontiguousarray(terms, F)
    n, d = terms.shape
    chunks = d // v
    lanes = lanes_of(chunks)
    trips = -(-chunks // lanes)
    padded = np.zeros((n, trips * lanes * v), F)
    padded[:, :d] = terms
    padded = padded.reshape(n, trips, lanes, v)
    s = np.zeros((n, lanes), F)
    started = np.zeros(lanes, bool)
    lane = np.arange(lanes)
    for it in range(trips):
        has = it * lanes + lane < chunks
        for k in range(v):
            m = padded[:, it, :, k]
            s = np.where(has, np.where(started, s + m, m), s)
            started = started | has
    off = lanes // 2
    while off:
        s = s + s[:, lane ^ off]
        off //= 2
    return s[:, 0].copy()


def rows_of(table, ids):
    """-> (the rows [N, d] with zeros where the id names no row, ok [N])"""
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < table.shape[0])
    x = np.asarray(table, F)[np.where(ok, ids, 0)]
    return np.where(ok[:, None], x, F(0)).astype(F), ok


class _Row(object):
    def __init__(self, table, ids, normalize, v):
        self.x, self.ok = rows_of(table, ids)
        n = self.x.shape[0]
        if normalize:
            self.ss = lane_sum(self.x * self.x, v)
            self.inv = F(1) / np.sqrt(np.where(self.ss > EPS, self.ss, EPS))
        else:
            self.ss, self.inv = np.zeros(n, F), np.ones(n, F)
        self.y = self.x * self.inv[:, None]


def _terms(kind, a, r, c):
    if kind == "distmult":
        return (a.y * r.y) * c.y
    e = (a.y + r.y) - c.y
    return np.abs(e) if kind == "trans_l1" else e * e


def _score(kind, a, r, c, v):
    s = lane_sum(_terms(kind, a, r, c), v)
    return -s if kind == "trans_l1" else -np.sqrt(s) if kind == "trans_l2" else s


def forward(ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize, v):
    """ent / rel: fp32 (widened) tables; neg [B, K] or None -> (pos [B], neg_out [B, K'])"""
    b = len(src)
    k = 0 if neg is None else np.asarray(neg).reshape(b, -1).shape[1]
    h, r, t = _Row(ent, src, normalize, v), _Row(rel, rel_id, normalize, v), _Row(ent, dst, normalize, v)
    pos = _score(kind, h, r, t, v)
    kp = 2 * k if corrupt == "both" else k
    out = np.zeros((b, kp), F)
    for j in range(k):
        n = _Row(ent, np.asarray(neg).reshape(b, k)[:, j], normalize, v)
        if corrupt != "tail":
            out[:, j] = _score(kind, n, r, t, v)
        if corrupt != "front":
            out[:, (k if corrupt == "both" else 0) + j] = _score(kind, h, r, n, v)
    return pos, out


def _contrib(kind, g, a, r, c, v):
    """what one scored triple adds to gy_a, gy_r, gy_c"""
    g = np.asarray(g, F)
    if kind == "distmult":
        gg = g[:, None]
        return gg * (r.y * c.y), gg * (a.y * c.y), gg * (a.y * r.y)
    e = (a.y + r.y) - c.y
    if kind == "trans_l1":
        gg = np.broadcast_to(g[:, None], e.shape)
        kk = np.where(e > 0, -gg, np.where(e < 0, gg, F(0))).astype(F)
    else:
        q = np.sqrt(lane_sum(e * e, v))
        with np.errstate(divide="ignore", invalid="ignore"):
            gq = np.where(q == 0, F(0), g / q).astype(F)
        kk = -(gq[:, None] * e)
    return kk, kk, -kk


def _row_grad(row, gy, normalize, v):
    if normalize:
        dot = lane_sum(row.y * gy, v)[:, None]
        inv = row.inv[:, None]
        gx = np.where((row.ss > EPS)[:, None], inv * (gy - row.y * dot), inv * gy)
    else:
        gx = gy
    return np.where(row.ok[:, None], gx, F(0)).astype(F)


def grad(ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize, v, g_pos, g_neg):
    """-> the per-occurrence gradients of the raw rows: G_src, G_rel, G_dst [B, d], G_neg [B, K, d]"""
    b, d = len(src), ent.shape[1]
    k = 0 if neg is None else np.asarray(neg).reshape(b, -1).shape[1]
    h, r, t = _Row(ent, src, normalize, v), _Row(rel, rel_id, normalize, v), _Row(ent, dst, normalize, v)
    gh, gr, gt = np.zeros((b, d), F), np.zeros((b, d), F), np.zeros((b, d), F)
    ca, cr, cc = _contrib(kind, g_pos, h, r, t, v)
    gh, gr, gt = gh + ca, gr + cr, gt + cc
    g_rows = np.zeros((b, k, d), F)
    g_neg = np.asarray(g_neg, F).reshape(b, -1) if k else None
    for j in range(k):
        n = _Row(ent, np.asarray(neg).reshape(b, k)[:, j], normalize, v)
        gn = np.zeros((b, d), F)
        if corrupt != "tail":
            ca, cr, cc = _contrib(kind, g_neg[:, j], n, r, t, v)
            gn, gr, gt = gn + ca, gr + cr, gt + cc
        if corrupt != "front":
            ca, cr, cc = _contrib(kind, g_neg[:, (k if corrupt == "both" else 0) + j], h, r, n, v)
            gh, gr, gn = gh + ca, gr + cr, gn + cc
        g_rows[:, j] = _row_grad(n, gn, normalize, v)
    return _row_grad(h, gh, normalize, v), _row_grad(r, gr, normalize, v), _row_grad(t, gt, normalize, v), g_rows


def scatter_rows(rows, keys, size):
    """fp32 scatter_add in input order (the order of ops.scatter_add): keys outside [0, size) drop out"""
    out = np.zeros((size, rows.shape[1]), F)
    for p, key in enumerate(np.asarray(keys, np.int64)):
        if 0 <= key < size:
            out[key] = out[key] + rows[p]
    return out


# ---- the float64 formulation of the reference's expressions --------------------------------
def _norm64(x, normalize):
    if not normalize:
        return x
    ss = (x * x).sum(-1, keepdims=True)
    return x / np.sqrt(np.maximum(ss, np.float64(EPS)))         # tf.nn.l2_normalize, epsilon = 1e-12f


def _score64(kind, a, r, c):
    """-> (score, the sum of the magnitudes of its terms)"""
    if kind == "distmult":
        p = a * r * c
        return p.sum(-1), np.abs(p).sum(-1)
    e = a + r - c
    mag = (np.abs(a) + np.abs(r) + np.abs(c)).sum(-1)
    if kind == "trans_l1":
        return -np.abs(e).sum(-1), mag
    return -np.sqrt((e * e).sum(-1)), mag


def forward64(ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize):
    """-> (pos, neg_out, mag_pos, mag_neg): float64 scores and the magnitude sums of their terms"""
    b = len(src)
    k = 0 if neg is None else np.asarray(neg).reshape(b, -1).shape[1]
    e64, r64 = np.asarray(ent, np.float64), np.asarray(rel, np.float64)

    def rows(table, ids):
        ids = np.asarray(ids, np.int64)
        ok = (ids >= 0) & (ids < table.shape[0])
        return _norm64(np.where(ok[..., None], table[np.where(ok, ids, 0)], 0.0), normalize)
    h, r, t = rows(e64, src), rows(r64, rel_id), rows(e64, dst)
    pos, mag_pos = _score64(kind, h, r, t)
    if k == 0:
        return pos, np.zeros((b, 0)), mag_pos, np.zeros((b, 0))
    n = rows(e64, np.asarray(neg).reshape(b, k))                 # [B, K, d]
    hh, rr, tt = h[:, None], r[:, None], t[:, None]              # the tile of transX.py:116-118
    front, tail = _score64(kind, n, rr, tt), _score64(kind, hh, rr, n)
    if corrupt == "front":
        return pos, front[0], mag_pos, front[1]
    if corrupt == "tail":
        return pos, tail[0], mag_pos, tail[1]
    return pos, np.concatenate([front[0], tail[0]], 1), mag_pos, np.concatenate([front[1], tail[1]], 1)


def forward_bound(kind, d, mag):
    return gamma(forward_n(kind, d)) * mag


# ---- the float64 gradient and the bound of the fp32 gradient's error -----------------------
GRAD_BOUND_NOTES = """
The bound of the gradient is propagated numerically beside the float64 gradient, every step by
the model above (n_y = d + 3 with normalize, else 0: y^ = y (1 + theta_{n_y})):
 contributions of one scored triple with upstream g (the same fp32 value on both sides):
   distmult  g (r c) etc.: two normalised factors, two products: err <= gamma(2 n_y + 2) |g r c|.
   trans     e^ = e + eta, |eta| <= E = gamma(n_y + 2) M.
     l1  -g sign(e): exact where |e| > E (the sign cannot differ), else err <= 2 |g|.
     l2  |q^ - q| <= Q = gamma(2d + 6) sum M (the forward bound).  Where q > Q:
         gq^ = fl(g / q^): dG = |g| Q / (q (q - Q)) + u |g| / (q - Q);
         err <= (|gq| + dG) E + dG |e| + u (|gq| + dG)(|e| + E).  Where q <= Q no bound exists (inf)
         - unless q is exactly 0 through identical rows, which the bit tests cover; g = 0 adds exactly 0.
 gy = the sum of J contributions, J - 1 roundings: dgy <= T + gamma(J - 1)(A + T), A = sum |term|,
   T = sum err.
 normalisation (ss > 1e-12): dot^ = sum fl(y^ gy^): dD <= sum |y| dgy + gamma(n_y) sum |y| (|gy| + dgy)
   + gamma(d) (1 + gamma(n_y)) sum |y| (|gy| + dgy);  inner = gy - y dot: dinner <= dgy + |y| dD +
   gamma(n_y + 1) |y| (|dot| + dD) + u (|gy| + dgy + (1 + gamma(n_y + 1)) |y| (|dot| + dD));
   gx = inv^ inner^, inv^ = inv (1 + theta_{d+2}), one product: dgx <= (1 + gamma(d+3)) inv dinner +
   gamma(d+3) inv |inner|.  ss <= 1e-12: the same with inner = gy.  (A row whose ss is within
   gamma(d) of the clamp could take the other branch: the test rows are far from it or exactly 0.)
 table: m occurrences added one by one: dtable <= sum dgx + gamma(m - 1) sum (|gx| + dgx), then one
   rounding to a 16-bit table: + max(u_t (|value| + dtable), s_t), u_t = 2^-8 (bf16) or 2^-11 (fp16) and
   s_t half the spacing of the type's subnormals, which bounds the rounding of a value below the
   smallest normal: 2^-25 for fp16 (values under 2^-14 = 6.1e-5 occur), nothing representable for bf16.
"""


def _times(a, b):
    """a * b for bounds that may be inf (no bound): 0 * inf is 0 - a zero factor is exactly zero"""
    with np.errstate(invalid="ignore"):
        p = a * b
    return np.where(np.isnan(p), 0.0, p)


def _row64(table, ids, normalize):
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < table.shape[0])
    x = np.where(ok[..., None], table[np.where(ok, ids, 0)], 0.0)
    if normalize:
        ss = (x * x).sum(-1, keepdims=True)
        inv = 1.0 / np.sqrt(np.maximum(ss, np.float64(EPS)))
    else:
        ss, inv = np.zeros(x.shape[:-1] + (1,)), np.ones(x.shape[:-1] + (1,))
    return dict(x=x, ok=ok, ss=ss, inv=inv, y=x * inv)


def _contrib64(kind, d, ny, g, a, r, c):
    """-> ((term_a, term_r, term_c), (err_a, err_r, err_c)) of one scored triple, float64"""
    g = np.asarray(g, np.float64)[..., None]
    a, r, c = a["y"], r["y"], c["y"]
    if kind == "distmult":
        terms = (g * (r * c), g * (a * c), g * (a * r))
        return terms, tuple(gamma(2 * ny + 2) * np.abs(t) for t in terms)
    e = a + r - c
    big_m = np.abs(a) + np.abs(r) + np.abs(c)
    big_e = gamma(ny + 2) * big_m
    if kind == "trans_l1":
        t = -g * np.sign(e)
        err = np.where(np.abs(e) > big_e, 0.0, 2 * np.abs(g)) * np.ones_like(e)
    else:
        q = np.sqrt((e * e).sum(-1, keepdims=True))
        big_q = gamma(2 * d + 6) * big_m.sum(-1, keepdims=True)
        safe = q > big_q
        qs, gap = np.where(safe, q, 1.0), np.where(safe, q - big_q, 1.0)
        gq = np.where(safe, g / qs, 0.0)
        dg = np.abs(g) * big_q / (qs * gap) + U * np.abs(g) / gap
        t = -gq * e
        err = (np.abs(gq) + dg) * big_e + dg * np.abs(e) + U * (np.abs(gq) + dg) * (np.abs(e) + big_e)
        err = np.where(safe | (np.asarray(g) == 0), err, np.inf) * np.ones_like(e)
    return (t, t, -t), (err, err, err)


class _Gy64(object):
    """gy of one row with the bound of its error: the sum, A = sum |term|, T = sum err, J"""

    def __init__(self, shape):
        self.g, self.a, self.t, self.j = np.zeros(shape), np.zeros(shape), np.zeros(shape), 0

    def add(self, term, err):
        self.g, self.a, self.t, self.j = self.g + term, self.a + np.abs(term), self.t + err, self.j + 1

    def bound(self):
        return self.t + gamma(max(self.j - 1, 0)) * (self.a + self.t)


def _row_grad64(row, gy, dgy, normalize, d, ny):
    if not normalize:
        gx, dgx = gy, dgy
    else:
        y, inv = np.abs(row["y"]), row["inv"]
        absg = np.abs(gy) + dgy
        dot = (row["y"] * gy).sum(-1, keepdims=True)
        yg = _times(y, absg).sum(-1, keepdims=True)
        dd = _times(y, dgy).sum(-1, keepdims=True) + gamma(ny) * yg + gamma(d) * (1 + gamma(ny)) * yg
        inner = gy - row["y"] * dot
        reach = _times(y, np.abs(dot) + dd)
        dinner = dgy + gamma(ny + 1) * reach + U * (absg + (1 + gamma(ny + 1)) * reach) + _times(y, dd)
        big = row["ss"] > np.float64(EPS)
        inner, dinner = np.where(big, inner, gy), np.where(big, dinner, dgy)
        gx = inv * inner
        dgx = (1 + gamma(d + 3)) * inv * dinner + gamma(d + 3) * inv * np.abs(inner)
    ok = row["ok"][..., None]
    return np.where(ok, gx, 0.0), np.where(ok, dgx, 0.0)


def grad64(ent, rel, src, rel_id, dst, neg, kind, corrupt, normalize, g_pos, g_neg):
    """the float64 per-occurrence gradients and the bounds of the fp32 ones' errors:
    -> [(G, dG) for src, rel, dst ([B, d]) and neg ([B, K, d])]"""
    b, d = len(src), ent.shape[1]
    k = 0 if neg is None else np.asarray(neg).reshape(b, -1).shape[1]
    ny = d + 3 if normalize else 0
    e64, r64 = np.asarray(ent, np.float64), np.asarray(rel, np.float64)
    h, r, t = _row64(e64, src, normalize), _row64(r64, rel_id, normalize), _row64(e64, dst, normalize)
    gh, gr, gt = _Gy64((b, d)), _Gy64((b, d)), _Gy64((b, d))
    terms, errs = _contrib64(kind, d, ny, g_pos, h, r, t)
    for acc, term, err in zip((gh, gr, gt), terms, errs):
        acc.add(term, err)
    out_n = (np.zeros((b, k, d)), np.zeros((b, k, d)))
    g_neg = np.asarray(g_neg, np.float64).reshape(b, -1) if k else None
    for j in range(k):
        n = _row64(e64, np.asarray(neg).reshape(b, k)[:, j], normalize)
        gn = _Gy64((b, d))
        if corrupt != "tail":
            terms, errs = _contrib64(kind, d, ny, g_neg[:, j], n, r, t)
            for acc, term, err in zip((gn, gr, gt), terms, errs):
                acc.add(term, err)
        if corrupt != "front":
            terms, errs = _contrib64(kind, d, ny, g_neg[:, (k if corrupt == "both" else 0) + j], h, r, n)
            for acc, term, err in zip((gh, gr, gn), terms, errs):
                acc.add(term, err)
        out_n[0][:, j], out_n[1][:, j] = _row_grad64(n, gn.g, gn.bound(), normalize, d, ny)
    return [_row_grad64(row, acc.g, acc.bound(), normalize, d, ny)
            for row, acc in ((h, gh), (r, gr), (t, gt))] + [out_n]


def table_grad64(rows, bounds, keys, size, unit_roundoff=0.0, half_spacing=0.0):
    """scatter_add of float64 gradient rows and of their bounds -> (table, bound); half_spacing:
    half the spacing of the dtype's subnormals - the absolute error of the rounding where the
    relative model does not hold (fp16: 2^-25, for |value| < 2^-14); unit_roundoff:
    of the table's dtype when the gradient is rounded to 16 bits"""
    keys = np.asarray(keys, np.int64)
    ok = (keys >= 0) & (keys < size)
    table, mag, err = (np.zeros((size, rows.shape[1])) for _ in range(3))
    np.add.at(table, keys[ok], rows[ok])
    np.add.at(err, keys[ok], bounds[ok])
    np.add.at(mag, keys[ok], np.abs(rows[ok]) + bounds[ok])
    m = np.bincount(keys[ok], minlength=size)[:, None]
    bound = err + np.where(m > 1, gamma(np.maximum(m - 1, 1)) * mag, 0.0)
    return table, bound + np.maximum(_times(unit_roundoff, np.abs(table) + bound), half_spacing)
