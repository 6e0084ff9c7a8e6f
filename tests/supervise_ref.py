"""The numpy restatement of euler_amd/csrc/supervise.h (the fused supervised loss head: sigmoid,
sigmoid cross-entropy with soft labels, its mean, floor(p + 0.5), tp / fp / fn / correct / total,
the two AUC histograms, the gradient): fp32 operations in the stated order, vectorised across rows;
the float64 formulation; the brute-force AUC (every prediction against every threshold); the
streaming metrics' formulas (utils/metrics.py:23-48 and tf.metrics.auc's ROC trapezoid); and the
error bound derived below.

Every numpy float32 ufunc used here (+, -, *, /, comparisons) is one correctly rounded operation,
so these loops and the header return the same bits.

ORDER.  row_loss[b] adds the terms of row b one by one, c = 0 .. C - 1, starting from the first;
the total is skipgram_ref.total with P + K = C (256 partials as a function of B alone, a butterfly
inside each run of 64, the four runs, one division by float(B * C)).

ERROR BOUND of the loss against float64 (u = 2^-24, gamma(n) = n u / (1 - n u); the logits and the
labels are inputs: exact).  With a = max(x, 0) - x z and L = log1p(exp(-|x|)) >= 0 the exact term
is a + L; a >= 0 for z in [0, 1], and |a| stands below so that a label outside [0, 1] (a graph's
feature slot may hold anything) is covered too.
 hard label (z in {0, 1}): a is exact (max(x, 0) or max(-x, 0)), and the term is skip-gram's:
        L^ = L (1 + theta), |theta| <= E_SP 2 u (skipgram_ref.E_SP, the measured ulp constant of the
        softplus; an ulp of the exact value is at most 2 u of it), or L^ = 0 with L <= SP_BELOW;
        the one add rounds once:  A = REL_TERM (|a| + L) + SP_BELOW,  REL_TERM = (1 + E_SP 2 u)(1 + u) - 1.
 soft label: ONE EXTRA PRODUCT, fl(x z) = x z (1 + d1), and ONE EXTRA ADD, a^ = fl(max(x, 0) -
        fl(x z)) = (max(x, 0) - x z (1 + d1)) (1 + d2), |d1|, |d2| <= u - half an ulp each:
        |a^ - a| <= da = u |x z| (1 + u) + u |a|.  Then the hard label's step on a^ + L:
        A = da + REL_TERM (|a| + da + L) + SP_BELOW.
 loss:  a term passes through at most C - 1 additions of its row, ceil(B / 256) of its partial and
        8 of the combine tree, then the rounding of float(B C) and the division;
        n = C + ceil(B / 256) + 9:   |loss^ - loss| <= (sum A + gamma(n) sum (|a| + L + A)) / (B C).
 gradient: p^ = sig(x) (1 + theta), |theta| <= REL_SIG (skipgram_ref), or p^ = 0 with sig < 2^-124;
        diff^ = fl(p^ - z): ddiff = REL_SIG sig + TINY + u (|sig - z| + REL_SIG sig + TINY);
        gs^ = g / N (1 + theta_2) (N and the division), the product rounds once:
        dg = |gs| (ddiff + gamma(3) (|sig - z| + ddiff)); a 16-bit gradient adds its one rounding.
"""
import numpy as np

import skipgram_ref as sg

F = np.float32
U = sg.U
EPS = 1e-7
gamma = sg.gamma
sigmoid = sg.sigmoid


def _relu(y):
    return np.where(y > 0, y, F(0)).astype(F)


def term_general(x, z):
    """(relu(x) - x * z) + Log1pUnit(exp(-|x|)): one multiply, two adds"""
    x, z = np.asarray(x, F), np.asarray(z, F)
    with np.errstate(invalid="ignore"):
        out = (_relu(x) - x * z) + sg.log1p_unit(sg.exp_of(x))
    assert out.dtype == F
    return out


def term(x, z):
    """hard labels through the two identities of the header (SgTerm), soft ones by the formula"""
    x, z = np.asarray(x, F), np.asarray(z, F)
    x, z = np.broadcast_arrays(x, z)
    return np.where(z == 0, sg.term(x, False), np.where(z == 1, sg.term(x, True), term_general(x, z))).astype(F)


def predict(p):
    return (np.asarray(p, F) + F(0.5)) >= F(1)


def thresholds(t):
    """tf.metrics.auc's table: Python floats, rounded once to fp32"""
    assert t >= 2
    return np.array([0.0 - EPS] + [i / (t - 1) for i in range(1, t - 1)] + [1.0 + EPS]).astype(F)


def bucket_brute(p, t):
    """the definition: the number of thresholds strictly below p, every p against every threshold"""
    return (thresholds(t)[None, :] < np.asarray(p, F).reshape(-1, 1)).sum(1).astype(np.int64)


def bucket(p, t):
    """the same number by bisection (the table is strictly increasing)"""
    return np.searchsorted(thresholds(t), np.asarray(p, F).reshape(-1), side="left").astype(np.int64)


def counts_of(p, z):
    """-> int64 [tp, fp, fn, correct, total]"""
    p, z = np.asarray(p, F).reshape(-1), np.asarray(z, F).reshape(-1)
    lab, pred = z != 0, predict(p)
    correct = z == pred.astype(F)
    return np.array([(lab & pred).sum(), (~lab & pred).sum(), (lab & ~pred).sum(), correct.sum(), p.size], np.int64)


def hist_of(p, z, t):
    """-> int64 [2, t + 1]: row 0 label != 0, row 1 label == 0"""
    p, z = np.asarray(p, F).reshape(-1), np.asarray(z, F).reshape(-1)
    bk, lab = bucket(p, t), z != 0
    return np.stack([np.bincount(bk[lab], minlength=t + 1), np.bincount(bk[~lab], minlength=t + 1)]).astype(np.int64)


def forward(x, z, t=None):
    """x, z: fp32 (widened) [B, C] -> dict(prob, diff, row_loss, loss, counts[, hist])"""
    x, z = np.asarray(x, F), np.asarray(z, F)
    b, c = x.shape
    p = sigmoid(x)
    tm = term(x, z)
    row_loss = np.zeros(b, F)
    for j in range(c):
        row_loss = tm[:, j] if j == 0 else row_loss + tm[:, j]
    out = dict(prob=p, diff=(p - z).astype(F), row_loss=row_loss.astype(F), loss=F(sg.total(row_loss, b, c, 0)),
               counts=counts_of(p, z))
    if t is not None:
        out["hist"] = hist_of(p, z, t)
    return out


def grad(diff, g, b, c):
    """-> the fp32 gradient of the logits before the rounding to their dtype"""
    gs = F(g) / sg.count(b, c, 0)
    return (gs * np.asarray(diff, F)).astype(F)


# ---- the streaming metrics -----------------------------------------------------------------
def f1_of(counts):
    """metrics.py:35-48"""
    tp, fp, fn = (float(v) for v in counts[:3])
    precision, recall = tp / (EPS + tp + fp), tp / (EPS + tp + fn)
    return 2.0 * precision * recall / (precision + recall + EPS)


def acc_of(counts):
    return float(counts[3]) / float(counts[4])


def _auc(tp, fn, fp, tn):
    tpr = (tp + EPS) / (tp + fn + EPS)
    fpr = fp / (fp + tn + EPS)
    return float(np.sum((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) / 2.0))


def confusion_from_hist(hist):
    """tp_i = the positives with bucket > i (p > thr_i): reverse cumulative sums -> tp, fn, fp, tn [T] float64"""
    hist = np.asarray(hist, np.int64)
    above = np.cumsum(hist[:, ::-1], axis=1)[:, ::-1][:, 1:]           # [2, T]: sum over k > i
    tp, fp = above[0], above[1]
    return tp.astype(np.float64), (hist[0].sum() - tp).astype(np.float64), fp.astype(np.float64), \
        (hist[1].sum() - fp).astype(np.float64)


def confusion_brute(p, z, t):
    """tf.metrics.auc literally: every prediction compared with every threshold"""
    p, z = np.asarray(p, F).reshape(-1), np.asarray(z, F).reshape(-1)
    lab = z != 0
    over = p[None, :] > thresholds(t)[:, None]                         # [T, n]
    tp, fp = (over & lab).sum(1), (over & ~lab).sum(1)
    return tp.astype(np.float64), (lab.sum() - tp).astype(np.float64), fp.astype(np.float64), \
        ((~lab).sum() - fp).astype(np.float64)


def auc_of(hist):
    return _auc(*confusion_from_hist(hist))


def auc_brute(p, z, t):
    return _auc(*confusion_brute(p, z, t))


# ---- the float64 formulation and the bounds -------------------------------------------------
REL_TERM = sg.REL_TERM
REL_SIG = sg.REL_SIG
SP_BELOW = sg.SP_BELOW
TINY = sg.TINY


def forward64(x, z):
    """-> (loss64, the bound of the fp32 loss's error)"""
    x, z = np.asarray(x, np.float64), np.asarray(z, np.float64)
    b, c = x.shape
    a = np.maximum(x, 0.0) - x * z
    big_l = np.log1p(np.exp(-np.abs(x)))
    soft = (z != 0) & (z != 1)
    da = np.where(soft, U * np.abs(x * z) * (1 + U) + U * np.abs(a), 0.0)
    err = da + REL_TERM * (np.abs(a) + da + big_l) + SP_BELOW
    n = c + -(-b // sg.PARTIALS) + 9
    return (a + big_l).sum() / (b * c), (err.sum() + gamma(n) * (np.abs(a) + big_l + err).sum()) / (b * c)


def grad64(x, z, g, unit=0.0, sub=0.0):
    """-> (the float64 gradient of the logits, the bound of the error of the computed one); unit /
    sub: the unit roundoff and half the subnormal spacing of a 16-bit gradient dtype"""
    x, z = np.asarray(x, np.float64), np.asarray(z, np.float64)
    n = x.size
    sig = sg._sigmoid64(x)
    m = sig - z
    ddiff = REL_SIG * sig + TINY + U * (np.abs(m) + REL_SIG * sig + TINY)
    gs = float(g) / n
    dg = abs(gs) * (ddiff + gamma(3) * (np.abs(m) + ddiff))
    want = gs * m
    return want, dg + unit * (np.abs(want) + dg) + sub
