"""The numpy restatement of euler_amd/csrc/skipgram.h (the fused skip-gram loss head of DeepWalk /
node2vec / LINE / unsupervised GraphSAGE): fp32 operations in the stated order, forward and
gradient, vectorised across pair rows; a literal restatement of the reference's metric
(utils/metrics.py:51-83); the float64 formulation (PosNegLogits + xent_loss of the reference);
and the error bounds derived below.

Every numpy float32 ufunc used here (+, -, *, /, comparisons) is one correctly rounded operation,
so these loops and the header return the same bits.

MEASURED CONSTANTS (tests/csrc/skipgram_check.cc, stride 1 over every fp32 value):
  E_L1P  the largest error of Log1pUnit(e) against log1p over every fp32 e in (0, 1], in ulps of
         the exact value (ulp(v) = 2^(floor(log2 v) - 23)).
  E_SP   the same for the whole softplus of a logit x in [-86, 0], Log1pUnit(ExpNonPositive(x))
         against log1p(exp(x)).  For x in [-90, -86) the result is +0 and the exact value is at
         most SP_BELOW = log1p(exp(-86)) < 2^-124: an absolute error, not a relative one.

ERROR BOUNDS (u = 2^-24, gamma(n) = n u / (1 - n u); Higham, Accuracy and Stability of Numerical
Algorithms, Lemma 3.1; the same value g on both sides).
 logit: one product and d - 1 additions in any order: |x^ - x| <= dx = gamma(d) sum |t_c c_c|.
 term:  softplus is 1-Lipschitz, so |sp(x^) - sp(x)| <= dx.  The computed term is
        fl(max(+-x^, 0) + L^), L^ = log1p(e) (1 + theta), |theta| <= E_SP 2 u (an ulp of the exact
        value is at most 2 u of it), or L^ = 0 with L <= SP_BELOW; both summands are >= 0 and the
        first is exact, so the sum has the relative error rel = (1 + E_SP 2 u)(1 + u) - 1:
        |term^ - sp(x)| <= A = dx + rel (sp(x) + dx) + SP_BELOW.
 loss:  a term passes through at most P + K - 1 additions of its row, ceil(B / 256) of its partial
        and 8 of the combine tree, then the rounding of float(B (P + K)) and the division;
        n = P + K + ceil(B / 256) + 9:   |loss^ - loss| <= (sum A + gamma(n) sum (sp(x) + A)) / N.
 sig:   the logistic function is 1/4-Lipschitz: |sig(x^) - sig(x)| <= dx / 4.  e^ = e (1 + theta),
        |theta| <= rho = E_EXP 2 u (edge_softmax_ref.E_ULP), or e^ = 0 with e < 2^-124; 1 + e^ and
        the quotient round once each; e / (1 + e) and 1 / (1 + e) move by at most the relative
        rho with e.  rs = (1 + u)^2 / (1 - rho)^2 - 1:  dsig = dx / 4 + rs sig(x) + 2^-124.
 c_j:   m = sig - 1 or sig; the subtraction rounds once: dm = dsig + u (|m| + dsig).  gs^ =
        g / N (1 + theta_2) (N and the division), the product rounds once:
        dc = |gs| (dm + gamma(3) (|m| + dm)).
 rows:  G_ctx_j = fl(c^ t): err <= dc |t| + u (|c| + dc) |t|.  G_src: P + K products, each rounded,
        P + K - 1 additions: T = sum dc_j |ctx_j|, A = sum |c_j| |ctx_j|:  err <= T + gamma(P + K)(A + T).
 table: triple_score_ref.table_grad64 (m occurrences added one by one, then one rounding to a
        16-bit table).
"""
import numpy as np

import edge_softmax_ref as smx
import triple_score_ref as kg

F = np.float32
U = 2.0 ** -24
DIMS = kg.DIMS
PARTIALS = 256
E_L1P = 1.9684        # (1.968361 at e = 0.00386178493, bit pattern 0x3b7d1600)
E_SP = 2.7970         # (2.796907 at x = -2.7570076, bit pattern 0xc03072d0)
SP_BELOW = float(np.log1p(np.exp(-86.0)))
gamma = kg.gamma
chunk_width = kg.chunk_width
lane_sum = kg.lane_sum
rows_of = kg.rows_of
scatter_rows = kg.scatter_rows
table_grad64 = kg.table_grad64

_Q = [F(1.0 / n) for n in (15, 13, 11, 9, 7, 5, 3)]


def log1p_unit(e):
    e = np.asarray(e, F)
    s = e / (F(2) + e)
    u = s * s
    q = np.full_like(s, _Q[0])
    for c in _Q[1:]:
        q = q * u + c
    s2 = s + s
    out = s2 + s2 * (u * q)
    assert out.dtype == F
    return out


def exp_of(x):
    return smx.exp_nonpositive(-np.abs(np.asarray(x, F)))


def term(x, positive):
    """softplus(-x) of a positive, softplus(x) of a negative"""
    x = np.asarray(x, F)
    y = -x if positive else x
    return np.where(y > 0, y, F(0)).astype(F) + log1p_unit(exp_of(x))


def sigmoid(x):
    x = np.asarray(x, F)
    e = exp_of(x)
    den = F(1) + e
    return np.where(x >= 0, F(1) / den, e / den).astype(F)


def count(b, p, k):
    return F(b * (p + k))


def coef(gs, x, positive):
    sig = sigmoid(x)
    return (F(gs) * ((sig + F(-1)) if positive else sig)).astype(F)


def total(row_loss, b, p, k):
    """the B row sums -> the loss: 256 partials, a butterfly inside each run of 64, the four runs"""
    if b == 0:
        return F(0)
    row_loss = np.asarray(row_loss, F)
    iters = -(-b // PARTIALS)
    pad = np.zeros(iters * PARTIALS, F)
    pad[:b] = row_loss
    part = np.zeros(PARTIALS, F)
    for i in range(iters):
        part = part + pad[i * PARTIALS:(i + 1) * PARTIALS]
    run = part.reshape(4, 64)
    lanes = np.arange(64)
    off = 32
    while off:
        run = run + run[:, lanes ^ off]
        off //= 2
    r = run[:, 0]
    return F((r[0] + r[1]) + (r[2] + r[3])) / count(b, p, k)


def _context_ids(pos, neg, b):
    pos = np.asarray(pos, np.int64).reshape(b, -1)
    if neg is None:
        return pos, pos.shape[1], 0
    neg = np.asarray(neg, np.int64).reshape(b, -1)
    return np.concatenate([pos, neg], 1), pos.shape[1], neg.shape[1]


def rank_of(logits, p):
    """the entries among the first P - 1 positives and the negatives that are >= the last positive"""
    x = np.asarray(logits, F)
    others = np.delete(x, p - 1, axis=1)
    return (others >= x[:, p - 1:p]).sum(1).astype(np.int32)


def forward(target, context, src, pos, neg, v):
    """target / context: fp32 (widened) tables -> (logits [B, P + K], rank [B] int32, row_loss [B], loss)"""
    b, d = len(src), target.shape[1]
    ids, p, k = _context_ids(pos, neg, b)
    t, _ = rows_of(target, src)
    logits = np.zeros((b, p + k), F)
    row_loss = np.zeros(b, F)
    for j in range(p + k):
        c, _ = rows_of(context, ids[:, j])
        logits[:, j] = lane_sum(t * c, v) if b else 0
        tj = term(logits[:, j], j < p)
        row_loss = tj if j == 0 else row_loss + tj
    return logits, rank_of(logits, p), row_loss.astype(F), total(row_loss, b, p, k)


def grad(target, context, src, pos, neg, logits, g, b_total=None):
    """-> the per-occurrence gradients of the raw rows: G_src [B, d], G_pos [B, P, d], G_neg [B, K, d];
    b_total: the B of the whole batch when the rows given are a selection of it"""
    b, d = len(src), target.shape[1]
    ids, p, k = _context_ids(pos, neg, b)
    t, t_ok = rows_of(target, src)
    gs = F(g) / count(b_total or b, p, k) if b else F(0)
    g_src = np.zeros((b, d), F)
    g_ctx = np.zeros((b, p + k, d), F)
    for j in range(p + k):
        c, c_ok = rows_of(context, ids[:, j])
        cj = coef(gs, logits[:, j], j < p)[:, None]
        g_src = g_src + cj * c
        g_ctx[:, j] = np.where(c_ok[:, None], cj * t, F(0))
    g_src = np.where(t_ok[:, None], g_src, F(0)).astype(F)
    return g_src, np.ascontiguousarray(g_ctx[:, :p]), np.ascontiguousarray(g_ctx[:, p:])


# ---- the reference's metric, literally -----------------------------------------------------
def mrr_score_ranks(logits, negative_logits):
    """metrics.py:51-61: all = concat([neg, pos], axis=2); size = shape(all)[2]; _, idx =
    top_k(all, k=size); _, ranks = top_k(-idx, k=size); the positive's rank = ranks[:, :, -1] + 1.
    logits [B, 1], negative_logits [B, K'] -> that rank minus one [B].  tf.nn.top_k orders equal
    values by increasing index, which a stable argsort of the negated values restates."""
    all_logits = np.concatenate([negative_logits, logits], axis=1)
    idx = np.argsort(-all_logits, axis=1, kind="stable")            # top_k(all, k=size) indices
    ranks = np.argsort(idx, axis=1, kind="stable")                  # top_k(-idx): where each entry stands
    return ranks[:, -1].astype(np.int32)


def metric(name, rank):
    rank = np.asarray(rank, np.float64)
    if name == "mrr":
        return float(np.mean(1.0 / (rank + 1.0)))
    if name == "mr":
        return float(np.mean(rank + 1.0))
    return float(np.mean(rank < int(name[3:])))


# ---- the float64 formulation and the bounds -------------------------------------------------
def _rows64(table, ids):
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < table.shape[0])
    return np.where(ok[..., None], np.asarray(table, np.float64)[np.where(ok, ids, 0)], 0.0), ok


def _softplus64(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid64(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


REL_TERM = (1 + E_SP * 2 * U) * (1 + U) - 1
RHO = smx.E_ULP * 2 * U
REL_SIG = (1 + U) ** 2 / (1 - RHO) ** 2 - 1
TINY = 2.0 ** -124


def forward64(target, context, src, pos, neg):
    """-> (logits64 [B, P + K], dx their bound, loss64, the bound of the fp32 loss's error)"""
    b, d = len(src), target.shape[1]
    ids, p, k = _context_ids(pos, neg, b)
    t, _ = _rows64(target, src)
    c, _ = _rows64(context, ids)                                   # [B, P + K, d]
    prod = t[:, None, :] * c
    x, dx = prod.sum(-1), gamma(d) * np.abs(prod).sum(-1)
    sign = np.where(np.arange(p + k) < p, -1.0, 1.0)
    sp = _softplus64(sign * x)
    n_terms = b * (p + k)
    a = dx + REL_TERM * (sp + dx) + SP_BELOW
    n = p + k + -(-b // PARTIALS) + 9
    return x, dx, sp.sum() / n_terms, (a.sum() + gamma(n) * (sp + a).sum()) / n_terms


def grad64(target, context, src, pos, neg, g):
    """the float64 per-occurrence gradients and the bounds of the fp32 ones' errors:
    -> [(G, dG) for src [B, d], pos [B, P, d], neg [B, K, d]]"""
    b, d = len(src), target.shape[1]
    ids, p, k = _context_ids(pos, neg, b)
    t, t_ok = _rows64(target, src)
    c, c_ok = _rows64(context, ids)
    x, dx, _, _ = forward64(target, context, src, pos, neg)
    sig = _sigmoid64(x)
    dsig = dx / 4 + REL_SIG * sig + TINY
    positive = (np.arange(p + k) < p)[None, :]
    m = np.where(positive, sig - 1.0, sig)
    dm = dsig + U * (np.abs(m) + dsig)
    gs = float(g) / (b * (p + k))
    cj = gs * m
    dc = abs(gs) * (dm + gamma(3) * (np.abs(m) + dm))
    g_ctx = cj[..., None] * t[:, None, :]
    d_ctx = (dc + U * (np.abs(cj) + dc))[..., None] * np.abs(t)[:, None, :]
    g_ctx, d_ctx = np.where(c_ok[..., None], g_ctx, 0.0), np.where(c_ok[..., None], d_ctx, 0.0)
    g_src = (cj[..., None] * c).sum(1)
    big_t, big_a = (dc[..., None] * np.abs(c)).sum(1), (np.abs(cj)[..., None] * np.abs(c)).sum(1)
    d_src = big_t + gamma(p + k) * (big_a + big_t)
    g_src, d_src = np.where(t_ok[:, None], g_src, 0.0), np.where(t_ok[:, None], d_src, 0.0)
    return [(g_src, d_src), (g_ctx[:, :p], d_ctx[:, :p]), (g_ctx[:, p:], d_ctx[:, p:])]
