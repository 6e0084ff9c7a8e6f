"""numpy restatement of euler_amd/csrc/mp_softmax.h: ExpNonPositive in np.float32 steps, and the
softmax / its gradient of a (segment, head) in the summation order the header states.  Every
operation below is one correctly rounded fp32 operation on float32 arrays (numpy never fuses).
Also the float64 formulas and the error bounds of DESIGN 4.11."""
import numpy as np

F = np.float32
SHORT, BLOCK = 32, 256
T = F(-86.0)                            # ExpNonPositive returns +0 below it
U = 2.0 ** -24
# E: the largest error of ExpNonPositive against the real exp, in ulps of the exact value
# (ulp(v) = 2^(floor(log2 v) - 23)), measured over EVERY fp32 value in [T, 0] by
# tests/csrc/edge_softmax_check.cc (smx_exp_error, stride 1): DESIGN 4.11.
E_ULP = 0.9568  # (0.956792 at d = -59.902615, bit pattern 0xc26f9c47)

_LOG2E = F(float.fromhex("0x1.715476p+0"))
_MAGIC = F(12582912.0)
_C1, _C2 = F(0.693359375), F(-2.12194440e-4)
_Q = [F(float.fromhex(h)) for h in ("0x1.a151a8p-13", "0x1.6d4352p-10", "0x1.1110c6p-7", "0x1.5554e8p-5",
                                    "0x1.555556p-3", "0x1.0p-1")]


def exp_nonpositive(d):
    d = np.asarray(d, F)
    with np.errstate(invalid="ignore"):
        live = d >= T
    x = np.where(live, d, F(0))
    t = x * _LOG2E + _MAGIC
    k = t.view(np.int32) - _MAGIC.view(np.int32)
    kf = t - _MAGIC
    r = x - kf * _C1
    r = r - kf * _C2
    q = np.full_like(r, _Q[0])
    for c in _Q[1:]:
        q = q * r + c
    p = F(1) + (r + (r * r) * q)
    assert p.dtype == F and r.dtype == F
    out = (p.view(np.int32) + k * np.int32(1 << 23)).view(F)
    return np.where(live, out, F(0))


def heads_per_wave(heads):
    return heads if heads <= 64 and 64 % heads == 0 else 1


def ordered_sum(terms, heads):
    """terms [S, n, H] float32 -> [S, H]: the SUM of mp_softmax.h along axis 1"""
    terms = np.asarray(terms, F)
    S, n, H = terms.shape
    if n <= SHORT:
        s = np.zeros((S, H), F)
        for p in range(n):
            s = s + terms[:, p]
        return s
    w = BLOCK // heads_per_wave(heads)
    iters = -(-n // w)
    pad = np.zeros((S, iters * w, H), F)            # (+0 added to a partial leaves its bits)
    pad[:, :n] = terms
    pad = pad.reshape(S, iters, w, H)
    part = np.zeros((S, w, H), F)
    for i in range(iters):
        part = part + pad[:, i]
    run = part.reshape(S, 4, w // 4, H)
    lanes = np.arange(w // 4)
    off = w // 8
    while off >= 1:
        run = run + run[:, :, lanes ^ off]
        off //= 2
    r = run[:, :, 0]
    return (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])


def forward_batch(x, heads):
    """x [S, n, H] float32 -> y, n >= 1"""
    x = np.asarray(x, F)
    m = x.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = exp_nonpositive(x - m)
    s = ordered_sum(e, heads)
    return e / s[:, None, :]


def backward_batch(y, g, heads):
    y, g = np.asarray(y, F), np.asarray(g, F)
    t = ordered_sum(y * g, heads)
    return y * (g - t[:, None, :])


def _by_length(seg_ptr):
    seg_ptr = np.asarray(seg_ptr, np.int64)
    lens = seg_ptr[1:] - seg_ptr[:-1]
    for n in np.unique(lens):
        if n > 0:
            starts = seg_ptr[:-1][lens == n]
            yield int(n), starts[:, None] + np.arange(n)[None, :]          # [S, n] positions


def edge_softmax_ref(x, seg_ptr, g=None):
    """the whole op on grouped data: x [E, H] (forward) or, with g, the gradient on y = x.
    Positions outside [seg_ptr[0], seg_ptr[-1]) are 0."""
    x = np.asarray(x, F)
    out = np.zeros_like(x)
    H = x.shape[1]
    for n, pos in _by_length(seg_ptr):
        out[pos] = forward_batch(x[pos], H) if g is None else backward_batch(x[pos], np.asarray(g, F)[pos], H)
    return out


def seg_ptr_of_sorted_keys(keys, size):
    """offsets of the destinations 0 .. size-1 in a non-decreasing key array"""
    return np.searchsorted(np.asarray(keys), np.arange(size + 1), side="left").astype(np.int64)


# ---- float64 formulas and the bounds of DESIGN 4.11 ------------------------------------------
def forward_f64(x, seg_ptr):
    x = np.asarray(x, np.float64)
    out = np.zeros_like(x)
    for n, pos in _by_length(seg_ptr):
        v = x[pos]
        e = np.exp(v - v.max(axis=1, keepdims=True))
        out[pos] = e / e.sum(axis=1, keepdims=True)
    return out


def forward_bound(x, seg_ptr, e_ulp):
    """|y^ - y| <= (y A u + (n + 1) exp(T)) / (1 - A u), A = |x_p - m| + max_q |x_q - m| + 4 E + n"""
    x = np.asarray(x, np.float64)
    y = forward_f64(x, seg_ptr)
    out = np.zeros_like(x)
    for n, pos in _by_length(seg_ptr):
        v = x[pos]
        dist = v.max(axis=1, keepdims=True) - v
        dist = np.where(np.isfinite(dist), dist, 0.0)               # (a -inf logit: y is exactly 0)
        a = dist + dist.max(axis=1, keepdims=True) + 4.0 * e_ulp + n
        out[pos] = (y[pos] * a * U + (n + 1) * np.exp(float(T))) / (1.0 - a * U)
    return out


def backward_f64(y, g, seg_ptr):
    y, g = np.asarray(y, np.float64), np.asarray(g, np.float64)
    out = np.zeros_like(y)
    for n, pos in _by_length(seg_ptr):
        t = (y[pos] * g[pos]).sum(axis=1, keepdims=True)
        out[pos] = y[pos] * (g[pos] - t)
    return out


def backward_bound(y, g, seg_ptr):
    """u |y_p| (n sum_q |y_q g_q| + 2 |g_p - t|) / (1 - n u)"""
    y, g = np.asarray(y, np.float64), np.asarray(g, np.float64)
    out = np.zeros_like(y)
    for n, pos in _by_length(seg_ptr):
        yg = y[pos] * g[pos]
        t = yg.sum(axis=1, keepdims=True)
        out[pos] = U * np.abs(y[pos]) * (n * np.abs(yg).sum(axis=1, keepdims=True) + 2 * np.abs(g[pos] - t)) \
            / (1.0 - n * U)
    return out


def exp_subsample():
    """the fixed subsample of [T, 0] on which E is re-measured: every 4099th bit pattern, and a
    window of 2048 patterns either side of every power of two and of T (as uint32 bit patterns
    of the negative floats -0.0 .. T)"""
    lo, hi = 0x80000000, int(np.array(T).view(np.uint32))
    parts = [np.arange(lo, hi + 1, 4099, dtype=np.int64)]
    for ex in range(-149, 7):
        c = int(np.array(F(-(2.0 ** ex))).view(np.uint32))
        parts.append(np.arange(c - 2048, c + 2049, dtype=np.int64))
    parts.append(np.arange(hi - 2048, hi + 1, dtype=np.int64))
    bits = np.unique(np.concatenate(parts))
    bits = bits[(bits >= lo) & (bits <= hi)]
    return bits.astype(np.uint32)


def ulp_error(got, d):
    """error of got (float32) against exp(d) in float64, in ulps of the exact value"""
    exact = np.exp(np.asarray(d, np.float64))
    ulp = 2.0 ** (np.floor(np.log2(exact)) - 23)
    return np.abs(np.asarray(got, np.float64) - exact) / ulp
