"""numpy restatement of euler_amd/csrc/mp_attention.h: the logit of every (update, head) in the
summation order the header states, the softmax of edge_softmax_ref.py, the ordered weighted fold,
and the destination side of the backward.  Every operation is one correctly rounded fp32 operation
on float32 arrays (numpy never fuses).  Also the float64 formulas and the bounds of DESIGN 4.20."""
import numpy as np

import edge_softmax_ref as es

F = np.float32
U = 2.0 ** -24


def chunk(dh):
    return 4 if dh % 4 == 0 else 1


def lanes(dh):
    chunks = dh // chunk(dh)
    l = 1
    while l < 64 and l < chunks:
        l *= 2
    return l


def dot(a, b):
    """a, b [N, dh] float32 -> [N]: DOT of mp_attention.h"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    n, dh = a.shape
    v, L = chunk(dh), lanes(dh)
    s = np.zeros((n, L), F)
    for j in range(dh // v):                      # chunk j belongs to partial j % L, in increasing j
        for c in range(j * v, j * v + v):
            s[:, j % L] = s[:, j % L] + a[:, c] * b[:, c]
    idx = np.arange(L)
    off = L // 2
    while off >= 1:
        s = s + s[:, idx ^ off]
        off //= 2
    return s[:, 0]


def rows_of(gi, n_rows):
    """the rows the kernels read: the low word as unsigned, clamped to the last row"""
    return np.minimum(np.asarray(gi, np.int64) & 0xFFFFFFFF, n_rows - 1)


def _dst(seg_ptr, e):
    """destination of every position (size where it has none)"""
    seg_ptr = np.asarray(seg_ptr, np.int64)
    size = len(seg_ptr) - 1
    pos = np.arange(e)
    d = np.searchsorted(seg_ptr, pos, side="right") - 1
    return np.where((pos < seg_ptr[0]) | (pos >= seg_ptr[-1]), size, d)


def logits(kind, q, k, gi, seg_ptr, heads, q_index=None, scale=1.0, slope=0.2):
    """[E, H] float32; 0 for positions outside the span of seg_ptr"""
    k = np.asarray(k, F)
    e = len(gi)
    size = len(seg_ptr) - 1
    dst = _dst(seg_ptr, e)
    live = dst < size
    out = np.zeros((e, heads), F)
    if not live.any():
        return out
    d = dst[live]
    qr = d if q_index is None else np.asarray(q_index, np.int64)[d]
    g = rows_of(gi, k.shape[0])[live]
    if kind == "dot":
        q = np.asarray(q, F)
        qr = np.minimum(qr, q.shape[0] - 1)
        dh = k.shape[1] // heads
        for h in range(heads):
            out[live, h] = F(scale) * dot(q[qr, h * dh:(h + 1) * dh], k[g, h * dh:(h + 1) * dh])
    else:
        qs = np.zeros((len(d), heads), F) if q is None else np.asarray(q, F)[np.minimum(qr, len(q) - 1)]
        a = qs + k[g]
        out[live] = np.where(a < 0, a * F(slope), a)
    return out


def fold(table, gi, w, seg_ptr, size):
    """out[r] = +0, then fl(acc + fl(table[g(p)] * w[p] expanded)) in increasing p"""
    table = np.asarray(table, F)
    w = np.asarray(w, F)
    dh = table.shape[1] // w.shape[1]
    rows = rows_of(gi, table.shape[0])
    out = np.zeros((size, table.shape[1]), F)
    seg_ptr = np.asarray(seg_ptr, np.int64)
    lens = seg_ptr[1:] - seg_ptr[:-1]
    for n, pos in es._by_length(seg_ptr):
        acc = np.zeros((pos.shape[0], table.shape[1]), F)
        for j in range(n):
            acc = acc + table[rows[pos[:, j]]] * np.repeat(w[pos[:, j]], dh, axis=1)
        out[lens == n] = acc
    return out


def forward(kind, q, k, v, gi, seg_ptr, heads, q_index=None, scale=1.0, slope=0.2):
    """-> (logits, alpha, out)"""
    size = len(seg_ptr) - 1
    x = logits(kind, q, k, gi, seg_ptr, heads, q_index, scale, slope)
    alpha = es.edge_softmax_ref(x, seg_ptr)
    return x, alpha, fold(k if v is None else v, gi, alpha, seg_ptr, size)


def backward(kind, q, k, v, gi, seg_ptr, heads, alpha, grad, q_index=None, scale=1.0, slope=0.2):
    """-> (ds [E, H], dq_dst [size, D])"""
    k = np.asarray(k, F)
    tv = k if v is None else np.asarray(v, F)
    grad = np.asarray(grad, F)
    e, size = len(gi), len(seg_ptr) - 1
    dst = _dst(seg_ptr, e)
    live = dst < size
    dvh = tv.shape[1] // heads
    da = np.zeros((e, heads), F)
    g = rows_of(gi, tv.shape[0])[live]
    for h in range(heads):
        if live.any():
            da[live, h] = dot(grad[dst[live], h * dvh:(h + 1) * dvh], tv[g, h * dvh:(h + 1) * dvh])
    ds = es.edge_softmax_ref(alpha, seg_ptr, da)
    if kind == "dot":
        ds = F(scale) * ds
        return ds, fold(k, gi, ds, seg_ptr, size)
    d = dst[live]
    qr = d if q_index is None else np.asarray(q_index, np.int64)[d]
    qs = np.zeros((len(d), heads), F) if q is None else np.asarray(q, F)[np.minimum(qr, len(q) - 1)]
    a = qs + k[rows_of(gi, k.shape[0])[live]]
    ds[live] = np.where(a < 0, ds[live] * F(slope), ds[live])
    dq = np.zeros((size, heads), F)
    seg_ptr = np.asarray(seg_ptr, np.int64)
    lens = seg_ptr[1:] - seg_ptr[:-1]
    for n, pos in es._by_length(seg_ptr):
        acc = np.zeros((pos.shape[0], heads), F)
        for j in range(n):
            acc = acc + ds[pos[:, j]]
        dq[lens == n] = acc
    return ds, dq


# ---- float64 formulas and the bounds of DESIGN 4.20 -------------------------------------------
def gamma(n):
    return n * U / (1.0 - n * U)


def logits_f64(kind, q, k, gi, seg_ptr, heads, q_index=None, scale=1.0, slope=0.2):
    """-> (the exact logits of the stored values, the bound on |fp32 logit - exact|), both [E, H]"""
    k = np.asarray(k, np.float64)
    e, size = len(gi), len(seg_ptr) - 1
    dst = _dst(seg_ptr, e)
    live = dst < size
    x = np.zeros((e, heads))
    bound = np.zeros((e, heads))
    d = dst[live]
    qr = d if q_index is None else np.asarray(q_index, np.int64)[d]
    g = rows_of(gi, k.shape[0])[live]
    if kind == "dot":
        q = np.asarray(q, np.float64)
        qr = np.minimum(qr, q.shape[0] - 1)
        dh = k.shape[1] // heads
        sc = float(F(scale))
        prod = (q[qr] * k[g]).reshape(len(d), heads, dh)
        exact = sc * prod.sum(-1)
        # the dot: gamma_dh * SUM |q_c k_c|; then one rounding for the scale
        x[live] = exact
        bound[live] = abs(sc) * gamma(dh) * np.abs(prod).sum(-1) * (1 + U) + U * np.abs(exact)
    else:
        qs = np.zeros((len(d), heads)) if q is None else np.asarray(q, np.float64)[np.minimum(qr, len(q) - 1)]
        a = qs + k[g]
        sl = float(F(slope))
        x[live] = np.where(a < 0, a * sl, a)
        # two roundings: the add, and the multiply by the slope where the value is negative
        bound[live] = np.where(a < 0, abs(sl) * U * np.abs(a) * (1 + U) + U * np.abs(a * sl), U * np.abs(a))
    return x, bound


def forward_f64(kind, q, k, v, gi, seg_ptr, heads, q_index=None, scale=1.0, slope=0.2):
    """-> (out in float64, the bound of DESIGN 4.20 on |fp32 out - it|), both [size, Dv]"""
    x, eps = logits_f64(kind, q, k, gi, seg_ptr, heads, q_index, scale, slope)
    tv = np.asarray(k if v is None else v, np.float64)
    size = len(seg_ptr) - 1
    dvh = tv.shape[1] // heads
    y = es.forward_f64(x, seg_ptr)
    rows = rows_of(gi, tv.shape[0])
    out = np.zeros((size, tv.shape[1]))
    bound = np.zeros((size, tv.shape[1]))
    seg_ptr = np.asarray(seg_ptr, np.int64)
    for r in range(size):
        b, en = int(seg_ptr[r]), int(seg_ptr[r + 1])
        n = en - b
        if n == 0:
            continue
        # the computed logits x^ lie within e = e_max (per head) of x.  Their exact softmax y^ lies
        # within y (exp(2 e) - 1) of y (numerator and denominator each move by a factor exp(+-e)),
        # and y^ <= y exp(2 e).  The kernel's softmax lies within the 4.11 B bound of y^:
        # (y^ A u + (n + 1) exp(T)) / (1 - A u) with A = |x^_p - m^| + max_q |x^_q - m^| + 4 E + n,
        # and |x^_p - m^| <= |x_p - m| + 2 e.
        e_max = eps[b:en].max(axis=0, keepdims=True)
        dist = x[b:en].max(axis=0, keepdims=True) - x[b:en]
        a = dist + dist.max(axis=0, keepdims=True) + 4.0 * es.E_ULP + n + 4.0 * e_max
        y_hi = y[b:en] * np.exp(2 * e_max)
        b411 = (y_hi * a * U + (n + 1) * np.exp(float(es.T))) / (1.0 - a * U)
        d_alpha = b411 + y[b:en] * (np.exp(2 * e_max) - 1)
        vals = tv[rows[b:en]]
        ye = np.repeat(y[b:en], dvh, axis=1)
        de = np.repeat(d_alpha, dvh, axis=1)
        out[r] = (vals * ye).sum(0)
        # the fold: n products and n sums of the computed alpha (<= y^ + B), then alpha's own error
        a_hi = np.repeat(y_hi + b411, dvh, axis=1)
        bound[r] = gamma(n) * (np.abs(vals) * a_hi).sum(0) + (np.abs(vals) * de).sum(0)
    return out, bound
