"""Exact models and statistics for the sampling-distribution tests (numpy only).

tests/test_sampling_distribution_gpu.py draws millions of ids from the HIP kernels and
tests/test_sampling_stats_host.py (a) shows, with numpy's own generator, that every case
of the GPU file accepts its exact distribution and rejects a planted bias at the same
`p`, `N` and statistic, and (b) runs the same battery on the CPU oracle.  Both import the
one case table below, so they cannot drift apart.

Level.  A statistic is accepted iff its p-value >= LEVEL = 1e-7: derived, not measured.
The GPU file computes about 1 300 statistics (one per motif row and case, plus the pooled
ones), so a correct sampler fails anywhere with probability <= 1.3e-4, and since every
run is deterministic that happens once or never.

Sizing.  N of a case is chosen so that noncentrality(p, q_planted, N) reaches
lambda_needed(df): the noncentrality at which a chi-square test at level 1e-7 has power
>= 1 - 1e-6 (table in lambda_needed).  The binding check is the host power test.

The replica design.  Most RNG streams are keyed by node id: one call
gives a node only `count` draws and duplicate roots get identical rows by contract.  So
a test graph is R disjoint copies of a small motif of M rows: copy r holds the nodes
x = r * M + j (ids base + stride * x, or an irregular map for the hashed lookup) and
points only into itself.  Every copy has the same rows (bit-identical running sums) but
different ids, hence different streams and one exact distribution; counts are pooled
over copies by motif position.  That is also what training relies on: independence
across node ids.

fp32 tables against fp64 models.  The neighbour models take the edge probabilities from
the stored fp32 running sums (the reference's definition, Node::Init), so they are exact
up to RandomSelect's own f32 `limit_end - limit_begin` (<= 6e-8 relative).  The alias
tables of sample_node / sample_root / sample_edge are built in fp32 and differ from the
fp64 w / sum(w) by about 1e-7 relative; at N <= 2e7 that is a noncentrality below 1e-3
against critical values above 28.  No tolerance is added for either.
"""
import math

import numpy as np

LEVEL = 1e-7
MIN_EXPECTED = 50


# ------------------------------------------------------------------ statistics
def _gamma_q(a, x):
    """Regularized upper incomplete gamma Q(a, x): series for x < a + 1, modified Lentz
    continued fraction beyond (which gives the tail itself, so it keeps its relative
    accuracy down to 1e-300)."""
    if x <= 0:
        return 1.0
    lg = -x + a * math.log(x) - math.lgamma(a)
    if x < a + 1.0:
        term = 1.0 / a
        s = term
        n = a
        for _ in range(100000):
            n += 1.0
            term *= x / n
            s += term
            if abs(term) < abs(s) * 1e-17:
                break
        return max(0.0, 1.0 - s * math.exp(lg))
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    for i in range(1, 100000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        if abs(d) < tiny:
            d = tiny
        c = b + an / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h * math.exp(lg) if lg > -745 else 0.0


def chi2_sf(x, df):
    """Survival function of the chi-square distribution with df degrees of freedom."""
    if df <= 0:
        return 1.0
    return _gamma_q(0.5 * df, 0.5 * float(x))


def lambda_needed(df):
    """Noncentrality at which a chi-square test of `df` degrees of freedom at level 1e-7
    has power >= 1 - 1e-6 (noncentral chi-square; tabulated at df = 2^k - 1 and read at
    the next tabulated df, which errs on the large side)."""
    for d, lam in ((1, 102), (3, 112), (15, 143), (63, 201), (255, 316), (1023, 544)):
        if df <= d:
            return lam
    raise ValueError("df beyond the table")


def merge_cells(expected, min_expected=MIN_EXPECTED):
    """Groups of adjacent cells whose expected counts reach min_expected: cells are
    merged with their neighbours in order, the remainder joins the last group.  No cell
    is dropped."""
    groups, cur, acc = [], [], 0.0
    for i, e in enumerate(expected):
        cur.append(i)
        acc += float(e)
        if acc >= min_expected:
            groups.append(cur)
            cur, acc = [], 0.0
    if cur:
        if groups:
            groups[-1].extend(cur)
        else:
            groups.append(cur)
    return groups


def gof(counts, p, min_expected=MIN_EXPECTED, N=None):
    """Pearson statistic of observed `counts` against exact probabilities `p` (fp64):
    returns (statistic, df, p-value).  Cells of p == 0 must hold 0 (asserted, not part of
    the statistic); cells of small expectation are merged, never dropped; counts.sum()
    must be N (the number of draws made; default: the sum itself)."""
    counts = np.asarray(counts, np.int64).reshape(-1)
    p = np.asarray(p, np.float64).reshape(-1)
    assert counts.shape == p.shape and (p >= 0).all()
    if N is None:
        N = int(counts.sum())
    assert int(counts.sum()) == int(N), "draws unaccounted for: %d of %d" % (counts.sum(), N)
    zero = p == 0
    assert (counts[zero] == 0).all(), \
        "ids of probability 0 were drawn: cells %s" % np.nonzero(zero & (counts > 0))[0].tolist()
    cp, cc = p[~zero], counts[~zero]
    groups = merge_cells(cp * N, min_expected)
    gp = np.array([cp[g].sum() for g in groups])
    gc = np.array([cc[g].sum() for g in groups], np.float64)
    assert abs(gp.sum() - 1.0) <= 1e-12, "merged probabilities sum to %r" % gp.sum()
    assert gc.sum() == N
    e = gp * N
    stat = float((((gc - e) ** 2) / e).sum())
    df = len(groups) - 1
    return stat, df, chi2_sf(stat, df)


def pair_independence(counts2d, p_row, p_col, min_expected=MIN_EXPECTED, N=None):
    """The same statistic for a k x k table of paired draws against the product of the
    exact marginals (row-major cells, the same merging rule): any dependence and any
    marginal bias moves it."""
    pr = np.asarray(p_row, np.float64)
    pc = np.asarray(p_col, np.float64)
    c = np.asarray(counts2d, np.int64)
    assert c.shape == (len(pr), len(pc))
    return gof(c.reshape(-1), np.outer(pr, pc).reshape(-1), min_expected, N)


def noncentrality(p, q, N):
    """N * sum (q - p)^2 / p: the noncentrality of Pearson's statistic when the data
    come from q (cells of p == 0 must have q == 0: they are a hard assertion instead)."""
    p = np.asarray(p, np.float64).reshape(-1)
    q = np.asarray(q, np.float64).reshape(-1)
    nz = p > 0
    assert (q[~nz] == 0).all()
    return float(N * (((q[nz] - p[nz]) ** 2) / p[nz]).sum())


# ------------------------------------------------------------------ planted biases
P_LIGHT_MIN = 1.0 / 160


def planted_marginal(p):
    """The biases a marginal case must reject, as {name: q}:
      light  the lightest entry of p >= 1/160 drawn 1.05 x too often (a row of equal
             nonzero entries: one entry x 1.02), the rest scaled down.  Entries lighter
             than 1/160 (the tails of the geometric and 1e-3-next-to-1e3 rows) would
             need N > 1e9 for a 5 % bias of their own; they are inside the statistic
             through the merged cells and the `first` / `last` biases cover the row ends
      first  the first nonzero entry never drawn
      last   0.6 % of all draws land on the last nonzero entry instead (a `u` that runs
             to the end of the row); where the row's last STORED entry has weight 0 the
             same fault draws an id of probability 0, which gof asserts on outright
    Rows of one nonzero entry have no bias to plant: every draw is that entry (gof's hard
    assertions)."""
    p = np.asarray(p, np.float64)
    nz = np.nonzero(p > 0)[0]
    if len(nz) < 2:
        return {}
    out = {}
    vals = p[nz]
    uniform = np.ptp(vals) <= 1e-12 * vals.max()
    ok = nz[vals >= P_LIGHT_MIN]
    i = int(ok[np.argmin(p[ok])]) if len(ok) else int(nz[np.argmax(vals)])
    f = 1.02 if uniform else 1.05
    q = p.copy()
    q[i] = min(p[i] * f, 1.0)
    rest = np.ones(len(p), bool)
    rest[i] = False
    q[rest] *= (1.0 - q[i]) / p[rest].sum()
    out["light"] = q
    q = p.copy()
    q[nz[0]] = 0.0
    out["first"] = q / q.sum()
    q = p * (1.0 - 0.006)
    q[nz[-1]] += 0.006
    out["last"] = q
    return out


def planted_pair(p_row, p_col, eps=0.005):
    """With probability eps the second draw repeats the first: q over the k x k cells."""
    pr = np.asarray(p_row, np.float64)
    pc = np.asarray(p_col, np.float64)
    assert len(pr) == len(pc)
    return (1.0 - eps) * np.outer(pr, pc) + eps * np.diag(pr)


# ------------------------------------------------------------------ motifs
class Motif:
    """rows[j][t] = (targets, weights): the type-t neighbour list of motif row j, targets
    as motif positions (the neighbour is the node at that position of the SAME copy)."""

    def __init__(self, rows, T, names=None):
        self.rows, self.T, self.M = rows, T, len(rows)
        self.names = names or ["row%d" % j for j in range(self.M)]
        seg = [0]
        tg, w = [], []
        for row in rows:
            assert len(row) == T
            for t in range(T):
                a, b = row[t]
                assert len(a) == len(b)
                tg += list(a)
                w += list(b)
                seg.append(len(tg))
        self.seg = np.asarray(seg, np.int64)            # [M * T + 1]
        self.tgt = np.asarray(tg, np.int64)
        self.w = np.asarray(w, np.float32)
        # Node::Init restated: sequential f32 running sums over the row (all types),
        # type_end relative to the row, type_prefix the running sum of the f32 type sums
        self.prefix = np.zeros(len(self.w), np.float32)
        self.type_end = np.zeros(self.M * T, np.int32)
        self.type_prefix = np.zeros(self.M * T, np.float32)
        for j in range(self.M):
            b, e = self.seg[j * T], self.seg[(j + 1) * T]
            self.prefix[b:e] = np.cumsum(self.w[b:e], dtype=np.float32)
            tsum = np.float32(0)
            for t in range(T):
                tb, te = self.seg[j * T + t], self.seg[j * T + t + 1]
                tw = np.float32(0)
                for x in self.w[tb:te]:
                    tw = np.float32(tw + x)
                tsum = np.float32(tsum + tw)
                self.type_end[j * T + t] = te - b
                self.type_prefix[j * T + t] = tsum

    def entry_probs(self, j, types):
        """Node::SampleNeighbor's distribution over the stored entries of row j for the
        listed edge types, literally (node.cc:98-161): one listed type draws in that
        type's segment by the running sums; 1 < k < T listed types draw the type by the
        differences of type_prefix over the LISTED types, then the entry; any other k
        (none listed, or k >= T) draws the type over all T.  None where the reference
        returns nothing (empty segment, zero type sum): the caller's default fill."""
        T = self.T
        b0 = self.seg[j * T]
        pre = self.prefix[b0:self.seg[(j + 1) * T]].astype(np.float64)
        te = self.type_end[j * T:(j + 1) * T]
        tp = self.type_prefix[j * T:(j + 1) * T].astype(np.float64)
        tw = np.diff(np.concatenate([[0.0], tp]))
        k = len(types)

        def within(t):
            b = 0 if t == 0 else int(te[t - 1])
            e = int(te[t])
            out = np.zeros(len(pre))
            if e <= b:
                return None
            lo = 0.0 if b == 0 else pre[b - 1]
            tot = pre[e - 1] - lo
            assert tot > 0, "a zero-weight segment listed alone is RandomSelect's fall-through"
            out[b:e] = np.diff(np.concatenate([[lo], pre[b:e]])) / tot
            return out

        if k == 1:
            return within(int(types[0]))
        if 1 < k < T:
            lt = [int(t) for t in types]
            s = sum(tw[t] for t in lt)
            if s == 0:
                return None
            ptype = [(t, tw[t] / s) for t in lt]
        else:
            if tp[T - 1] == 0:
                return None
            ptype = [(t, tw[t] / tp[T - 1]) for t in range(T)]
        out = np.zeros(len(pre))
        for t, pt in ptype:
            if pt > 0:
                out += pt * within(t)
        return out

    def model(self, j, types):
        """entry_probs pooled by neighbour id (motif position): p [M] or None."""
        pe = self.entry_probs(j, types)
        if pe is None:
            return None
        b, e = self.seg[j * self.T], self.seg[(j + 1) * self.T]
        return np.bincount(self.tgt[b:e], weights=pe, minlength=self.M)

    def sorted_lists(self):
        """The same rows with every (row, type) list in ascending id order."""
        rows = []
        for row in self.rows:
            r = []
            for a, b in row:
                o = np.argsort(np.asarray(a), kind="stable")
                r.append(([a[i] for i in o], [b[i] for i in o]))
            rows.append(r)
        return Motif(rows, self.T, self.names)


def plain_motif(mild=False, cap=16):
    """M = 16 rows, one edge type; every kind of row the issue lists.  mild: the geometric
    row stops at 2^-9 (10 entries fit one bucket of the weight-bucket index).  The full row
    overflows its bucket, which makes the library decline the index for the lean fanout
    kernels (wb_lean_ok: more than 2 buckets in a thousand overflow) - the full motif
    reaches the pivot-level and second-chance paths, the mild one the index paths.  cap = 9:
    no row segment of more than nine entries falls into one bucket, so the header + window
    side index that hop 2 of the plain fanout draws through (wb_hw2.h: nine entries per
    line) is built as well."""
    rng = np.random.default_rng(1601)
    rows = [
        (list(range(16)), [float(i + 1) for i in range(16)]),            # weights 1..16 (+ self-loop)
        (list(range(2, 10)), [1.0] * 8),                                  # uniform 8 (no self-loop)
        (list(range(min(10, cap))), [0, 3, 0, 1, 2, 0, 0, 5, 1, 0] if cap >= 10 else [0, 3, 0, 1, 2, 0, 5, 1, 0]),   # zeros, first and last too
        ([5], [2.5]),                                                     # a single neighbour
        ([], []),                                                         # no neighbours
        (list(range(min(10 if mild else 16, cap))), [2.0 ** -i for i in range(min(10 if mild else 16, cap))]),   # geometric
        ([1, 2, 3, 6, 7, 9], [1e3, 1e-3, 1e3, 1e-3, 1e-3, 1e3]),          # 1e-3 next to 1e3
        ([3, 9, 3, 12], [1, 2, 3, 4]),                                    # a repeated neighbour id
        ([8, 2], [1, 3]),                                                 # a self-loop
    ]
    names = ["w1..16", "uniform8", "zeros", "single", "empty", "geometric", "1e-3|1e3",
             "repeated", "selfloop"]
    while len(rows) < 16:
        d = min(int(rng.integers(2, 13)), cap)
        rows.append((rng.permutation(16)[:d].tolist(), (rng.random(d) * 7.5 + 0.5).round(3).tolist()))
        names.append("random%d" % len(rows))
    # every position is somebody's neighbour (hop 2 and the walks reach every row)
    return Motif([[r] for r in rows], 1, names)


def typed_motif():
    """M = 16 rows, T = 3: an empty type, a zero-weight type, a dominating type."""
    rng = np.random.default_rng(1603)
    rows = [
        [([0, 1, 2, 3], [1, 2, 3, 4]), ([4, 5, 6, 7], [1, 1, 1, 1]), ([8, 9, 10], [5, 1, 1])],
        [([], []), ([11, 12, 13], [1, 2, 3]), ([14, 15], [4, 4])],                    # empty type 0
        [([0, 5], [1, 2]), ([6, 7], [0, 0]), ([8, 1, 2], [3, 1, 2])],                 # zero-weight type 1
        [([3, 4], [1000, 500]), ([9], [1]), ([10, 11], [0.5, 0.5])],                  # type 0 dominates
        [([], []), ([], []), ([], [])],                                               # no neighbours
    ]
    names = ["three", "emptytype0", "zerotype1", "dominant0", "empty"]
    while len(rows) < 16:
        perm = rng.permutation(16)
        rows.append([(perm[0:3].tolist(), [1, 2, 3]), (perm[3:5].tolist(), [2, 2]),
                     (perm[5:9].tolist(), (rng.random(4) * 4 + 0.5).round(3).tolist())])
        names.append("mixed%d" % len(rows))
    return Motif(rows, 3, names)


def uniform_motif(T):
    """Every weight 1.0 (the library's uniform-weight builds): row j lists the 8 positions
    after it, split over T types as evenly as they go."""
    rows = []
    for j in range(16):
        tg = [(j + 1 + i) % 16 for i in range(8)]
        cut = [8 * t // T for t in range(T + 1)]
        rows.append([(tg[cut[t]:cut[t + 1]], [1.0] * (cut[t + 1] - cut[t])) for t in range(T)])
    return Motif(rows, T, ["uniform8"] * 16)


HUB_M, HUB_DEG, HUB_MID = 8192, 6000, 600


def hub_motif():
    """M = 8192 rows: row 0 (the hub) has 6 000 entries, each its own neighbour, of
    heavy-tailed (Pareto) weights - long enough for the weight-bucket index's second-chance
    path and for pivot levels deeper than one block; rows 1 and 2 have 600 entries each and
    point mostly at each other and at the hub (repeated ids: pooled), so node2vec's child
    and parent lists span several 256-entry chunks; every other row is two entries that
    lead back to the long rows.  Lists are in random (storage) order."""
    rng = np.random.default_rng(1607)
    rows = [(rng.permutation(np.arange(16, 16 + HUB_DEG)).tolist(),
             ((rng.pareto(1.2, HUB_DEG) + 1) * 0.5).astype(np.float32).tolist())]
    for j in (1, 2):
        tg = np.where(rng.random(HUB_MID) < 0.7, rng.choice([0, 1, 2], HUB_MID), rng.integers(3, HUB_M, HUB_MID))
        rows.append((tg.tolist(), (rng.random(HUB_MID) * 3 + 0.1).astype(np.float32).tolist()))
    for j in range(3, HUB_M):
        rows.append(([1 + j % 2, 0], [1.0, 1.0]))
    return Motif([[r] for r in rows], 1, ["hub6000", "mid600a", "mid600b"] + ["short"] * (HUB_M - 3))


def equal_mass_bins(p, n_bins):
    """Map of cells to n_bins bins of (nearly) equal expected mass, in cell order."""
    c = np.cumsum(p) / np.sum(p)
    return np.minimum((c * n_bins - 1e-12).astype(np.int64).clip(0), n_bins - 1)


class Replicas:
    """R disjoint copies of a motif as raw adjacency for O.csr_from_raw / Graph.from_csr.
    layout 'copy': x = r * M + j (copies contiguous); 'row': x = j * R + r (the same
    motif row at neighbouring ids).  id = base + stride * x + (x & 1 if jitter): with
    jitter the ids are no arithmetic sequence, so the library maps them through its hash
    table instead of the strided identity."""

    def __init__(self, motif, R, base=1, stride=1, jitter=False, layout="copy"):
        assert base >= 1 and (not jitter or stride >= 3)
        self.motif, self.R, self.base, self.stride = motif, R, base, stride
        self.jitter, self.layout = jitter, layout
        self.M, self.T = motif.M, motif.T
        self.n = R * self.M

    def id_of_x(self, x):
        x = np.asarray(x, np.int64)
        return self.base + self.stride * x + ((x & 1) if self.jitter else 0)

    def x_of(self, j, r):
        return r * self.M + j if self.layout == "copy" else j * self.R + r

    def ids_of_row(self, j):
        return self.id_of_x(self.x_of(j, np.arange(self.R, dtype=np.int64)))

    def raw(self):
        """(row_id, seg_ptr, nbr, w) in x order."""
        m, M, T, R = self.motif, self.M, self.T, self.R
        x = np.arange(self.n, dtype=np.int64)
        j = x % M if self.layout == "copy" else x // R
        r = x // M if self.layout == "copy" else x % R
        deg = np.diff(m.seg)                                  # per (row, type)
        segdeg = deg.reshape(M, T)[j].reshape(-1)
        seg = np.zeros(self.n * T + 1, np.int64)
        seg[1:] = np.cumsum(segdeg)
        rowdeg = segdeg.reshape(self.n, T).sum(1)
        E = int(seg[-1])
        owner = np.repeat(x, rowdeg)                          # row of every entry
        within = np.arange(E, dtype=np.int64) - np.repeat(seg[::T][:-1], rowdeg)
        src = m.seg[j[owner] * T] + within                    # entry in the motif arrays
        tgt_x = self.x_of(m.tgt[src], r[owner])
        return (self.id_of_x(x).astype(np.uint64), seg, self.id_of_x(tgt_x).astype(np.uint64),
                m.w[src].copy())

    # decoding on the device or the host: works on numpy arrays and torch tensors alike
    def x_from_id(self, ids):
        return (ids - self.base) // self.stride

    def pos_from_x(self, x):
        return x % self.M if self.layout == "copy" else x // self.R


# ------------------------------------------------------------------ node / edge / label / layer models
def node_sampler_model(node_type, node_weight, types):
    """sample_node over node types: w / sum(w) within one type; type -1 draws the type by
    its weight sum first; a list draws the type among the listed SET by weight sum
    (graph.cc:221-275).  Which is w / (sum over the drawn-from types) per node."""
    nt = np.asarray(node_type)
    w = np.asarray(node_weight, np.float64)
    types = list(np.atleast_1d(types))
    n_types = int(nt.max()) + 1
    sel = range(n_types) if types == [-1] else sorted(set(int(t) for t in types))
    tsum = {t: w[nt == t].sum() for t in sel}
    tot = sum(tsum.values())
    p = np.zeros(len(w))
    for t in sel:
        if tsum[t] > 0:
            p[nt == t] = (tsum[t] / tot) * (w[nt == t] / tsum[t])
    return p


def n2v_weights(child_ids, child_w, parent_ids, parent_id, p, q):
    """RWCallback::BuildWeights (random_walk_op.cc:140-168), literally: a two-cursor walk
    over the child and parent lists AS STORED; f32 weights divided by the f32 q or p.  On
    ascending lists this is node2vec; on storage-order lists it is the reference's quirk
    (a child found in the parent's list is only recognised while the cursors agree)."""
    w = np.asarray(child_w, np.float32).copy()
    p32, q32 = np.float32(p), np.float32(q)
    j = k = 0
    nc, npar = len(child_ids), len(parent_ids)
    while j < nc and k < npar:
        if child_ids[j] < parent_ids[k]:
            w[j] = w[j] / (q32 if child_ids[j] != parent_id else p32)
            j += 1
        elif child_ids[j] == parent_ids[k]:
            k += 1
            j += 1
        else:
            k += 1
    while j < nc:
        w[j] = w[j] / (q32 if child_ids[j] != parent_id else p32)
        j += 1
    return w


def n2v_model(motif, prev, cur, p, q, first_step=False, variant=None):
    """Distribution of the next position for a walker that came from `prev` and stands on
    `cur` (motif positions; ids are monotone in the position inside a copy, so comparing
    positions is comparing ids).  first_step: the parent list is empty and parent = the
    start node itself.  CompactWeightedCollection::Init's f32 running sums are restated.
    variant 'swapped' / 'undivided' are the planted faults (p and q exchanged; the return
    weight left undivided)."""
    T = motif.T
    cb, ce = motif.seg[cur * T], motif.seg[(cur + 1) * T]
    c_ids, c_w = motif.tgt[cb:ce], motif.w[cb:ce]
    if first_step:
        par_ids, parent_id = np.zeros(0, np.int64), cur
    else:
        par_ids, parent_id = motif.tgt[motif.seg[prev * T]:motif.seg[(prev + 1) * T]], prev
    if ce == cb:
        return None
    if variant == "swapped":
        p, q = q, p
    w = n2v_weights(c_ids, c_w, par_ids, parent_id, p, q)
    if variant == "undivided":
        w0 = n2v_weights(c_ids, c_w, par_ids, parent_id, 1.0, q)
        w = np.where(c_ids == parent_id, w0, w).astype(np.float32)
    sums = np.cumsum(w, dtype=np.float32).astype(np.float64)
    pe = np.diff(np.concatenate([[0.0], sums])) / sums[-1]
    return np.bincount(c_ids, weights=pe, minlength=motif.M)


def local_layer_model(ids, w, t, weight_func):
    """API_LOCAL_SAMPLE_L: the distinct (id, type) candidates of a batch row, duplicate
    weights added (f32), then weight_func: 'sqrt' takes the square root, any other name
    leaves the sum (local_layer_host.h: take_sqrt).  Returns ({(id, type): p})."""
    acc = {}
    for i, x, tt in zip(ids, w, t):
        acc[(int(i), int(tt))] = np.float32(acc.get((int(i), int(tt)), np.float32(0)) + np.float32(x))
    if weight_func == "sqrt":
        acc = {k: np.sqrt(np.float32(v)) for k, v in acc.items()}
    tot = sum(float(v) for v in acc.values())
    return {k: float(v) / tot for k, v in acc.items()}


# ------------------------------------------------------------------ the case table
# Sizes.  R copies x count draws x calls per motif row; the +5 % bias on the lightest
# of weights 1..16 (p = 1/136) has noncentrality 1.9e-5 N, so that row needs N >= 7.6 M
# at df = 15; every marginal case below gives each row N = 8.4 M (8.3 M at odd counts).
R_GPU = 32768
SEED = 0x5EED0001               # base seed of every case; recheck seeds are SEED + 1 .. SEED + 4
RECHECK_SEEDS = (SEED + 1, SEED + 2, SEED + 3, SEED + 4)

GRAPHS = {
    # name: (motif factory, replica arguments)
    "plain": (plain_motif, dict(base=1)),
    "hashed": (plain_motif, dict(base=1000, stride=3, jitter=True)),
    "mild": (lambda: plain_motif(True), dict(base=1)),
    "hashedmild": (lambda: plain_motif(True), dict(base=1000, stride=3, jitter=True)),
    "side": (lambda: plain_motif(True, 9), dict(base=1)),
    "typed": (typed_motif, dict(base=1)),
    "uniform": (lambda: uniform_motif(1), dict(base=1)),
    "utyped": (lambda: uniform_motif(3), dict(base=1)),
    "rowmajor": (plain_motif, dict(base=1, layout="row")),
    "sorted": (lambda: plain_motif().sorted_lists(), dict(base=1)),
    "hub": (hub_motif, dict(base=1)),
    "hubsorted": (lambda: motif_of("hub").sorted_lists(), dict(base=1)),
}
_MOTIFS = {}


def motif_of(graph):
    if graph not in _MOTIFS:
        _MOTIFS[graph] = GRAPHS[graph][0]()
    return _MOTIFS[graph]


def replicas(graph, R):
    return Replicas(motif_of(graph), R, **GRAPHS[graph][1])


# Marginal cases of the neighbour draw.  per_call = draws per motif row and call, as a
# multiple of R; N per row = R * per_call * calls.  call_id: the first call id; call c
# of a case uses call_id + stride * c (stride = the ids one call consumes).
NEIGHBOR_CASES = [
    # name, graph, entry, types, count(s), calls, call_id, extra
    dict(name="nb_plain_tf_even", graph="plain", entry="neighbor", types=[0], count=64, calls=4, call_id=100, layout="tf"),
    dict(name="nb_plain_core_odd", graph="plain", entry="neighbor", types=[0], count=63, calls=4, call_id=110, layout="core"),
    dict(name="nb_hashed_tf_odd", graph="hashed", entry="neighbor", types=[0], count=63, calls=4, call_id=120, layout="tf"),
    dict(name="nb_hashed_core_even", graph="hashed", entry="neighbor", types=[0], count=64, calls=4, call_id=130, layout="core"),
    dict(name="nb_typed_one", graph="typed", entry="neighbor", types=[2], count=64, calls=4, call_id=140, layout="tf"),
    dict(name="nb_typed_several", graph="typed", entry="neighbor", types=[0, 2], count=64, calls=4, call_id=150, layout="tf"),
    dict(name="nb_typed_several_odd", graph="typed", entry="neighbor", types=[2, 1], count=63, calls=4, call_id=160, layout="core"),
    dict(name="nb_typed_none_listed", graph="typed", entry="neighbor", types=[], count=64, calls=4, call_id=170, layout="tf"),
    dict(name="nb_uniform", graph="uniform", entry="neighbor", types=[0], count=64, calls=4, call_id=180, layout="tf"),
    dict(name="nb_utyped_several", graph="utyped", entry="neighbor", types=[0, 1], count=63, calls=4, call_id=190, layout="tf"),
    dict(name="sets_typed", graph="typed", entry="sets", types=[[0], [0, 2], [0, 1, 2]], count=64, calls=4, call_id=200),
    # sample_fanout [8, 8]: 8 draws per root and hop, so 32 calls for the same N
    dict(name="fanout_plain", graph="plain", entry="fanout", types=[[0], [0]], count=[8, 8], calls=32, call_id=1000,
         kernel="SampleFanoutLeanKernel"),
    dict(name="fanout_mild", graph="mild", entry="fanout", types=[[0], [0]], count=[8, 8], calls=32, call_id=1050,
         kernel="SampleFanoutPlainKernel"),
    dict(name="fanout_side", graph="side", entry="fanout", types=[[0], [0]], count=[8, 8], calls=32, call_id=1075,
         kernel="SampleFanoutPlainKernel", side=2),
    dict(name="fanout_hashed", graph="hashed", entry="fanout", types=[[0], [0]], count=[8, 8], calls=32, call_id=1100,
         kernel="SampleFanoutLocalKernel"),
    dict(name="fanout_hashedmild", graph="hashedmild", entry="fanout", types=[[0], [0]], count=[8, 8], calls=32,
         call_id=1150, kernel="SampleFanoutLeanKernel"),
    dict(name="fanout_typed_one", graph="typed", entry="fanout", types=[[0], [2]], count=[8, 8], calls=32, call_id=1200,
         kernel="SampleFanoutLeanKernel"),
    dict(name="fanout_typed_several", graph="typed", entry="fanout", types=[[0, 2], [2, 1]], count=[8, 8], calls=32,
         call_id=1300, kernel="SampleFanoutLeanKernel"),
    dict(name="fanout_typed_several_lds", graph="typed", entry="fanout", types=[[0, 2], [2, 1]], count=[8, 8], calls=32,
         call_id=1400, kernel="SampleFanoutLeanKernel", tuning=(48, 0, 1)),
    dict(name="fanout_uniform", graph="uniform", entry="fanout", types=[[0], [0]], count=[8, 8], calls=32, call_id=1500,
         kernel="SampleFanoutLeanKernel"),
    dict(name="fanout_utyped_one", graph="utyped", entry="fanout", types=[[1], [0]], count=[8, 8], calls=32, call_id=1600,
         kernel="SampleFanoutLeanKernel"),
    dict(name="fanout_utyped_several", graph="utyped", entry="fanout", types=[[0, 1], [1, 2]], count=[8, 8], calls=32,
         call_id=1700, kernel="SampleFanoutLeanKernel"),
    # sample_fanout_multi: 8 tiles per call, each its own pair of call ids
    dict(name="multi_plain", graph="mild", entry="multi", types=[[0], [0]], count=[8, 8], calls=4, tiles=8, call_id=2000),
    dict(name="multi_typed", graph="typed", entry="multi", types=[[0, 2], [2, 1]], count=[8, 8], calls=4, tiles=8,
         call_id=2100),
]
# hop 2 of a fanout draws once per DISTINCT hop-1 id (duplicates share their row by
# contract), so its N per row is the number of distinct parents of that row times the
# count.  The roots of a call are all M nodes of every copy, each its own stream, so the
# node at position k is somebody's hop-1 child with probability
# 1 - prod_j (1 - p_j(k))^c1 exactly; the case is sized with that binomial's mean less 8
# of its standard deviations (lower_bound) and the test asserts the observed N reaches it.
def lower_bound(trials, prob):
    """Mean - 8 sd of Binomial(trials, prob), floored at 0: what a sized N may count on."""
    return max(0, int(trials * prob - 8.0 * math.sqrt(trials * prob * (1.0 - prob))))


def hop2_hit_probability(case):
    m = motif_of(case["graph"])
    miss = np.ones(m.M)
    for j in range(m.M):
        p = m.model(j, case["types"][0])
        if p is not None:
            miss *= (1.0 - p) ** case["count"][0]
    return 1.0 - miss


def case_rows(case, R=R_GPU):
    """The statistics of a neighbour-draw case as a list of dicts {label, hop, row, types,
    p (None: every output is the default fill), N}: N is exact for hop 1 and the sized
    lower bound for hop 2 (the test asserts the observed N reaches it and uses the
    observed one)."""
    m = motif_of(case["graph"])
    out = []
    if case["entry"] in ("neighbor", "sets"):
        tsets = case["types"] if case["entry"] == "sets" else [case["types"]]
        for s, ts in enumerate(tsets):
            for j in range(m.M):
                out.append(dict(label="%s/set%d/%s" % (case["name"], s, m.names[j]), hop=s, row=j, types=ts,
                                p=m.model(j, ts), N=R * case["count"] * case["calls"]))
        return out
    tiles = case.get("tiles", 1)
    hit = hop2_hit_probability(case)
    for h in range(2):
        for j in range(m.M):
            n = R * case["count"][h] * case["calls"] * tiles
            out.append(dict(label="%s/hop%d/%s" % (case["name"], h + 1, m.names[j]), hop=h, row=j,
                            types=case["types"][h], p=m.model(j, case["types"][h]),
                            N=n if h == 0 else lower_bound(n // case["count"][1], hit[j]) * case["count"][1]))
    return out


# sample_node / sample_n_with_types: 48 nodes of 3 types on three copies of the plain
# motif (type = copy): weights 1..16; uniform; zeros first and last around a geometric run
NODE_TYPES = np.repeat(np.arange(3), 16).astype(np.int32)
NODE_WEIGHTS = np.concatenate([np.arange(1, 17), np.full(16, 2.5),
                               [0, 8, 4, 2, 1, 1, 1, 3, 3, 0, 0, 5, 7, 2, 6, 0]]).astype(np.float32)
NODE_CASES = [
    dict(name="node_one_type", types=[0], count=1 << 23, call_id=3000),
    dict(name="node_one_type_zeros", types=[2], count=1 << 23, call_id=3001),
    dict(name="node_all_types", types=[-1], count=3 << 23, call_id=3002),
    dict(name="node_type_list", types=[0, 2], count=3 << 22, call_id=3003),
]
NWT_TYPES = [0, 1, 2, -1]           # sample_n_with_types: rows cycle through these
NWT_ROWS, NWT_COUNT, NWT_CALL = 4 * 4096, 4096, 3100          # N = 16.8 M per listed type

# edge / label draws: one record per motif entry of copy 0 of the typed graph
LABELS = 37
LABEL_COUNT, LABEL_CALL = 1 << 25, 3300
EDGE_COUNT, EDGE_CALL = 1 << 24, 3200


def typed_edge_records():
    """(src, dst, type, weight) of the distinct (src, dst, type) entries of the typed
    motif, ids = position + 1."""
    m = motif_of("typed")
    src, dst, ty, w = [], [], [], []
    for j in range(m.M):
        for t in range(m.T):
            a, b = m.rows[j][t]
            for x, y in zip(a, b):
                src.append(j + 1)
                dst.append(x + 1)
                ty.append(t)
                w.append(y)
    return (np.asarray(src, np.uint64), np.asarray(dst, np.uint64), np.asarray(ty, np.int32),
            np.asarray(w, np.float32))


def edge_model(types, weights, edge_type):
    """sample_edge: w / sum(w) within the type; -1 draws the type by its weight sum first."""
    return node_sampler_model(types, weights, [edge_type])


# walks with p = q = 1 (a count-1 neighbour draw keyed by the current node and
# call_id + step): N per row is the number of distinct (call, step, node) - at least the
# R start nodes per call
WALK_CASES = [
    dict(name="walk_plain_merged", graph="plain", walkers="all", walk_len=8, calls=256, call_id=5000),
    dict(name="walk_plain_per_walker", graph="plain", walkers="quarter", walk_len=8, calls=1024, call_id=9000),
    dict(name="walk_hashed_merged", graph="hashed", walkers="all", walk_len=8, calls=256, call_id=20000),
]

# node2vec: walkers are their own streams.  W walkers start on every node of the rows
# N2V_STARTS, two steps; step 1 and step 2 are judged separately
N2V_STARTS = (0, 7, 9)
N2V_PER_NODE = 8
N2V_PQ = ((0.25, 4.0), (2.0, 0.5))
N2V_CALL = 40000

# independence: k = 8 cells on the uniform-8 row (cell = position) and on the weights
# 1..16 row (cell = position // 2)
PAIR_ROWS = {"uniform8": (1, 1, 2), "w1..16": (0, 2, 0)}   # name: (motif row, positions per cell, first position)
PAIR_EPS = 0.005
PAIR_MIN_N = 1_200_000


def pair_marginal(row_name):
    j, per, off = PAIR_ROWS[row_name]
    p = motif_of("plain").model(j, [0])
    out = p[off:off + 8 * per].reshape(8, per).sum(1)
    assert abs(out.sum() - 1.0) < 1e-12
    return out


# ------------------------------------------------------------------ reports
class Report:
    """Collects one line per statistic and prints the table a run ends with."""

    def __init__(self):
        self.lines = []

    def add(self, label, stat, df, N, pv):
        self.lines.append((label, stat, df, int(N), pv))
        print("%-46s chi2 = %10.2f  df = %4d  N = %10d  p = %.3e" % (label, stat, df, N, pv))

    def failures(self):
        return [l for l in self.lines if not l[4] >= LEVEL]


def judge_rows(report, label, table, rows_p, rows_N, min_expected=MIN_EXPECTED):
    """table [rows, cells + 1] (last column: default fills).  Per row: a row without a
    model must be all default fills, every other row none; gof per row, then the pooled
    statistic (sum of the rows' statistics and dfs).  Returns the failing labels."""
    bad = []
    tot, tdf, tn = 0.0, 0, 0
    for j, (p, N) in enumerate(zip(rows_p, rows_N)):
        row = np.asarray(table[j])
        if p is None:
            assert row[:-1].sum() == 0 and row[-1] == N, "%s row %d: expected %d default fills, got %s" % (
                label, j, N, row.tolist())
            continue
        assert row[-1] == 0, "%s row %d: %d default fills on a row that has neighbours" % (label, j, row[-1])
        stat, df, pv = gof(row[:-1], p, min_expected, N)
        report.add("%s/row%d" % (label, j), stat, df, N, pv)
        if not pv >= LEVEL:
            bad.append("%s/row%d" % (label, j))
        tot, tdf, tn = tot + stat, tdf + df, tn + N
    pv = chi2_sf(tot, tdf)
    report.add("%s/pooled" % label, tot, tdf, tn, pv)
    if not pv >= LEVEL:
        bad.append("%s/pooled" % label)
    return bad


# ------------------------------------------------------------------ runners
# One implementation of every case for both backends: euler_amd.Graph (tensors on the
# GPU; the counting happens there and only the count tables come back) and OracleBackend
# below (the CPU oracle behind the same method names, torch CPU tensors).  torch is
# imported by the callers and handed in, so that importing this module needs numpy only.
class OracleBackend:
    """oracle.OracleGraph behind the call signatures of euler_amd.Graph.  The entries the
    oracle does not have as one call (sample_neighbor_sets, sample_fanout_multi, the auto
    call-id counter) are composed from the call ids DESIGN section 3 gives them."""

    def __init__(self, torch, OG):
        self.torch, self.OG, self.seed, self._call_id = torch, OG, 0, 0

    def set_seed(self, seed, call_id=0):
        self.seed, self._call_id = int(seed), int(call_id)

    def _take(self, n, call_id):
        if call_id is not None:
            return int(call_id)
        c = self._call_id
        self._call_id += n
        return c

    def _t(self, a, dt=np.int64):
        return self.torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt)))

    def sample_neighbor(self, nodes, edge_types, count, default_node=-1, layout="tf", call_id=None):
        nd = nodes.numpy().astype(np.int64)
        cid = self._take(1, call_id)
        if layout == "tf":
            on, _, _ = self.OG.sample_neighbor(self.seed, cid, nd, edge_types, count, default_node)
        else:
            _, on, _, _ = self.OG.sample_neighbor_core(self.seed, cid, nd.astype(np.uint64), edge_types, count)
        return self._t(on).reshape(len(nd), count), None, None

    def sample_neighbor_sets(self, nodes, type_sets, count, default_node=-1, call_id=None):
        cid = self._take(len(type_sets), call_id)
        return self.torch.stack([self.sample_neighbor(nodes, ts, count, default_node, "tf", cid + s)[0]
                                 for s, ts in enumerate(type_sets)], 0), None, None

    def sample_fanout(self, nodes, edge_types, counts, default_node=-1, call_id=None):
        cid = self._take(len(counts), call_id)
        on, _, _ = self.OG.sample_fanout(self.seed, cid, nodes.numpy(), edge_types, list(counts), default_node)
        return [nodes] + [self._t(a) for a in on], None, None

    def sample_fanout_multi(self, batches, edge_types, counts, default_node=-1, call_id=None):
        cid = self._take(len(counts) * len(batches), call_id)
        return [self.sample_fanout(b, edge_types, counts, default_node, cid + i * len(counts))
                for i, b in enumerate(batches)]

    def sample_node(self, count, node_type=-1, call_id=None):
        return self._t(self.OG.sample_node(self.seed, self._take(1, call_id), node_type, count))

    def sample_n_with_types(self, count, types, call_id=None):
        return self._t(self.OG.sample_n_with_types(self.seed, self._take(1, call_id), types, count))

    def random_walk(self, nodes, edge_types, p=1.0, q=1.0, default_node=-1, call_id=None):
        L = len(edge_types)
        return self._t(self.OG.random_walk(self.seed, self._take(max(L, 1), call_id), nodes.numpy(),
                                           edge_types, L, p, q, default_node))


def _decode(torch, rep, ids, default):
    """(motif position with M for a default fill, x) of every id; every other id must be
    a node of the graph."""
    isdef = ids == default
    x = torch.where(isdef, torch.zeros_like(ids), rep.x_from_id(ids))
    assert int(x.min()) >= 0 and int(x.max()) < rep.n, "an id outside the graph was drawn"
    back = rep.base + rep.stride * x + ((x & 1) if rep.jitter else 0)
    assert bool((isdef | (back == ids)).all()), "an id that is no node of the graph was drawn"
    pos = torch.where(isdef, torch.full_like(ids, rep.M), rep.pos_from_x(x))
    return pos, x


def _copy_of(rep, x):
    return x // rep.M if rep.layout == "copy" else x % rep.R


def tally(torch, rep, root_x, ids, default):
    """Counts [M, M + 1] of (motif row of the root, motif position of the id | default fill)
    for ids [n, c] drawn for the roots root_x [n]; ids must lie in the root's own copy."""
    M = rep.M
    pos, x = _decode(torch, rep, ids, default)
    same = _copy_of(rep, x) == _copy_of(rep, root_x)[:, None]
    assert bool(((pos == M) | same).all()), "a neighbour outside the root's copy was drawn"
    key = rep.pos_from_x(root_x)[:, None] * (M + 1) + pos
    return torch.bincount(key.reshape(-1), minlength=M * (M + 1)).reshape(M, M + 1).cpu().numpy()


def _all_roots(torch, rep, device):
    x = torch.arange(rep.n, dtype=torch.int64, device=device)
    return x, rep.base + rep.stride * x + ((x & 1) if rep.jitter else 0)


def _first_occurrence(torch, keys, valid, size):
    """first[k] = the smallest flat index i with keys[i] == k and valid[i] (else `big`)."""
    big = keys.numel()
    idx = torch.arange(big, dtype=torch.int64, device=keys.device)
    first = torch.full((size,), big, dtype=torch.int64, device=keys.device)
    first.scatter_reduce_(0, keys[valid], idx[valid], "amin")
    return first, big


def fanout_tables(torch, rep, root_x, nb, counts, default=-1):
    """One sample_fanout result -> (hop-1 table, hop-2 table, distinct parents per motif
    row, first, h1, h2).  Hop 2 is keyed by the hop-1 id, so all occurrences of one id
    must carry the same row (asserted) and ONE of them is counted."""
    n, c1, c2 = root_x.numel(), counts[0], counts[1]
    h1, h2 = nb[1].reshape(n, c1), nb[2].reshape(n * c1, c2)
    t1 = tally(torch, rep, root_x, h1, default)
    par = h1.reshape(-1)
    valid = par != default
    ppos, px = _decode(torch, rep, par, default)
    first, big = _first_occurrence(torch, px, valid, rep.n)
    assert torch.equal(h2[valid], h2[first[px[valid]]]), "duplicate hop-1 ids with different hop-2 rows"
    assert bool((h2[~valid] == default).all()), "a hop-2 row under a default hop-1 id"
    sel = first[first < big]
    t2 = tally(torch, rep, px[sel], h2[sel], default)
    parents = torch.bincount(ppos[sel], minlength=rep.M + 1)[:rep.M].cpu().numpy()
    return t1, t2, parents, first, h1, h2


def run_neighbor_case(B, torch, device, rep, case, seed, report, calls=None):
    """Runs one case of NEIGHBOR_CASES on backend B and judges it; returns the failing labels."""
    calls = calls or case["calls"]
    m, M, R = rep.motif, rep.M, rep.R
    root_x, roots = _all_roots(torch, rep, device)
    B.set_seed(seed)
    bad = []
    if case["entry"] == "neighbor":
        default = -1 if case["layout"] == "tf" else 0
        t = np.zeros((M, M + 1), np.int64)
        for c in range(calls):
            ids = B.sample_neighbor(roots, case["types"], case["count"], -1, layout=case["layout"],
                                    call_id=case["call_id"] + c)[0]
            t += tally(torch, rep, root_x, ids, default)
        N = R * case["count"] * calls
        return judge_rows(report, case["name"], t, [m.model(j, case["types"]) for j in range(M)], [N] * M)
    if case["entry"] == "sets":
        S = len(case["types"])
        t = np.zeros((S, M, M + 1), np.int64)
        for c in range(calls):
            ids = B.sample_neighbor_sets(roots, case["types"], case["count"], -1, call_id=case["call_id"] + S * c)[0]
            for s in range(S):
                t[s] += tally(torch, rep, root_x, ids[s], -1)
        N = R * case["count"] * calls
        for s, ts in enumerate(case["types"]):
            bad += judge_rows(report, "%s/set%d" % (case["name"], s), t[s], [m.model(j, ts) for j in range(M)], [N] * M)
        return bad
    c1, c2 = case["count"]
    tiles = case.get("tiles", 1)
    t1, t2, par = np.zeros((M, M + 1), np.int64), np.zeros((M, M + 1), np.int64), np.zeros(M, np.int64)
    for c in range(calls):
        cid = case["call_id"] + 2 * tiles * c
        if case["entry"] == "fanout":
            res = [B.sample_fanout(roots, case["types"], [c1, c2], -1, call_id=cid)]
        else:
            res = B.sample_fanout_multi([roots] * tiles, case["types"], [c1, c2], -1, call_id=cid)
        for nb, _, _ in res:
            a, b, p, _, _, _ = fanout_tables(torch, rep, root_x, nb, (c1, c2))
            t1, t2, par = t1 + a, t2 + b, par + p
    N1 = R * c1 * calls * tiles
    bad += judge_rows(report, case["name"] + "/hop1", t1, [m.model(j, case["types"][0]) for j in range(M)], [N1] * M)
    sized = [r["N"] for r in case_rows(dict(case, calls=calls), R) if r["hop"] == 1]
    for j in range(M):
        assert par[j] * c2 >= sized[j], "%s hop 2 row %d: %d draws, sized for %d" % (case["name"], j, par[j] * c2, sized[j])
    bad += judge_rows(report, case["name"] + "/hop2", t2, [m.model(j, case["types"][1]) for j in range(M)],
                      [int(x) * c2 for x in par])
    return bad


def run_walk_case(B, torch, device, rep, case, seed, report, calls=None):
    """random_walk with p = q = 1.  A step is a count-1 neighbour draw keyed by the CURRENT
    NODE and call_id + step (walk_kernels.hip), so walkers standing on one
    node at one step take the same move: asserted, and one transition is counted per
    distinct (call, step, node).  Transition counts are pooled over steps and calls."""
    calls = calls or case["calls"]
    m, M, L = rep.motif, rep.M, case["walk_len"]
    root_x, roots = _all_roots(torch, rep, device)
    if case["walkers"] == "quarter":
        root_x, roots = root_x[:rep.n // 4], roots[:rep.n // 4]
    n = roots.numel()
    B.set_seed(seed)
    t, seen = np.zeros((M, M + 1), np.int64), np.zeros(M, np.int64)
    step = torch.arange(L, dtype=torch.int64, device=device)[None, :]
    for c in range(calls):
        w = B.random_walk(roots, [[0]] * L, 1.0, 1.0, -1, call_id=case["call_id"] + L * c)
        cur, nxt = w[:, :-1].reshape(-1), w[:, 1:].reshape(-1)
        valid = cur != -1
        cpos, cx = _decode(torch, rep, cur, -1)
        key = (step * rep.n + cx.reshape(n, L)).reshape(-1)
        first, big = _first_occurrence(torch, key, valid, L * rep.n)
        assert torch.equal(nxt[valid], nxt[first[key[valid]]]), "walkers on one node at one step moved apart"
        assert bool((nxt[~valid] == -1).all()), "a walker that left the graph came back"
        sel = first[first < big]
        t += tally(torch, rep, cx[sel], nxt[sel][:, None], -1)
        seen += torch.bincount(cpos[sel], minlength=M + 1)[:M].cpu().numpy()
    sized = (rep.R if case["walkers"] == "all" else rep.R // 4) * calls
    assert (seen >= sized).all(), (seen, sized)
    return judge_rows(report, case["name"], t, [m.model(j, [0]) for j in range(M)], [int(x) for x in seen])


def n2v_starts(torch, rep, device, per_node):
    ids = np.concatenate([np.repeat(rep.ids_of_row(j), per_node) for j in N2V_STARTS])
    return torch.as_tensor(ids.astype(np.int64), device=device)


def n2v_expected_rows(motif, p, q, walkers_per_start_row):
    """[(label, prev or None, cur, model, sized N)]: step 1 per start row, step 2 per
    (start, first move) of positive probability, sized with lower_bound of the walkers that make that first move."""
    rows = []
    for s in N2V_STARTS:
        p1 = n2v_model(motif, None, s, p, q, first_step=True)
        rows.append(("step1/%d" % s, None, s, p1, walkers_per_start_row))
        for cur in np.nonzero(p1 > 0)[0]:
            rows.append(("step2/%d>%d" % (s, cur), s, int(cur), n2v_model(motif, s, int(cur), p, q),
                         lower_bound(walkers_per_start_row, p1[cur])))
    return rows


def run_n2v_case(B, torch, device, rep, p, q, seed, report, per_node, label):
    """node2vec, two steps from many walkers per start node (streams are walker indices,
    so walkers on one node are independent): step 1 (empty parent list, parent = the start
    node) and step 2 ((prev, cur) -> next) against BuildWeights restated."""
    M = rep.M
    starts = n2v_starts(torch, rep, device, per_node)
    B.set_seed(seed)
    w = B.random_walk(starts, [[0], [0]], p, q, -1, call_id=N2V_CALL)
    p0, x0 = _decode(torch, rep, w[:, 0], -1)
    p1, x1 = _decode(torch, rep, w[:, 1], -1)
    p2, x2 = _decode(torch, rep, w[:, 2], -1)
    c0 = _copy_of(rep, x0)
    assert bool(((p1 == M) | (_copy_of(rep, x1) == c0)).all()) and bool(((p2 == M) | (_copy_of(rep, x2) == c0)).all())
    t1 = torch.bincount(p0 * (M + 1) + p1, minlength=M * (M + 1)).reshape(M, M + 1).cpu().numpy()
    t2 = torch.bincount((p0 * (M + 1) + p1) * (M + 1) + p2, minlength=M * (M + 1) ** 2) \
        .reshape(M, M + 1, M + 1).cpu().numpy()
    bad, tot, tdf, tn = [], 0.0, 0, 0
    for name, prev, cur, model, sized in n2v_expected_rows(rep.motif, p, q, rep.R * per_node):
        row = t1[cur] if prev is None else t2[prev, cur]
        N = int(row.sum())
        assert N >= sized, (label, name, N, sized)
        if model is None:
            assert row[-1] == N
            continue
        assert row[-1] == 0
        stat, df, pv = gof(row[:-1], model, MIN_EXPECTED, N)
        report.add("%s/%s" % (label, name), stat, df, N, pv)
        if not pv >= LEVEL:
            bad.append("%s/%s" % (label, name))
        tot, tdf, tn = tot + stat, tdf + df, tn + N
    pv = chi2_sf(tot, tdf)
    report.add(label + "/pooled", tot, tdf, tn, pv)
    if not pv >= LEVEL:
        bad.append(label + "/pooled")
    return bad


# ---- independence: every runner returns {row name: (k x k table, N)}
PAIR_CALL = 60000


def _cells(torch, rep, ids, cell):
    per, off = cell
    pos, _ = _decode(torch, rep, ids, -1)
    c = (pos - off) // per
    assert bool(((c >= 0) & (c < 8)).all())
    return c


def _pair_table(torch, a, b):
    return torch.bincount((a * 8 + b).reshape(-1), minlength=64).reshape(8, 8).cpu().numpy()


def _row_roots(torch, rep, device, j):
    r = torch.arange(rep.R, dtype=torch.int64, device=device)
    x = r * rep.M + j if rep.layout == "copy" else j * rep.R + r
    return x, rep.base + rep.stride * x + ((x & 1) if rep.jitter else 0)


def pairs_draws(B, torch, device, rep, seed, parity, calls=2):
    """Draws d and d + 1 of one root: even d = the two halves of one Philox block, odd d =
    the last half of one block and the first of the next."""
    out = {}
    for name, (j, *per) in PAIR_ROWS.items():
        _, roots = _row_roots(torch, rep, device, j)
        B.set_seed(seed)
        t = np.zeros((8, 8), np.int64)
        for c in range(calls):
            cell = _cells(torch, rep, B.sample_neighbor(roots, [0], 64, -1, call_id=PAIR_CALL + c)[0], per)
            a, b = (cell[:, 0::2], cell[:, 1::2]) if parity == 0 else (cell[:, 1:63:2], cell[:, 2:64:2])
            t += _pair_table(torch, a, b)
        out[name] = (t, int(t.sum()))
    return out


def pairs_calls_or_seeds(B, torch, device, rep, seed, what):
    """The same root and draw under call ids c and c + 1, or under seeds s and s + 1."""
    out = {}
    for name, (j, *per) in PAIR_ROWS.items():
        _, roots = _row_roots(torch, rep, device, j)
        B.set_seed(seed)
        a = _cells(torch, rep, B.sample_neighbor(roots, [0], 64, -1, call_id=PAIR_CALL + 10)[0], per)
        if what == "seeds":
            B.set_seed(seed + 1)
        b = _cells(torch, rep, B.sample_neighbor(roots, [0], 64, -1,
                                                 call_id=PAIR_CALL + (11 if what == "calls" else 10))[0], per)
        t = _pair_table(torch, a, b)
        out[name] = (t, int(t.sum()))
    return out


def pairs_ids(B, torch, device, rep, seed, calls=2):
    """Node ids x and x + 1, same call and draw: rep is the row-major layout, where the
    nodes of one motif row have consecutive ids."""
    assert rep.layout == "row" and rep.stride == 1
    out = {}
    for name, (j, *per) in PAIR_ROWS.items():
        _, roots = _row_roots(torch, rep, device, j)
        B.set_seed(seed)
        t = np.zeros((8, 8), np.int64)
        for c in range(calls):
            cell = _cells(torch, rep, B.sample_neighbor(roots, [0], 64, -1, call_id=PAIR_CALL + 20 + c)[0], per)
            t += _pair_table(torch, cell[0::2], cell[1::2])
        out[name] = (t, int(t.sum()))
    return out


def _rows_of(torch, rep, first, big, h2, xs):
    """The hop-2 rows of the nodes xs (where they were somebody's hop-1 child) and the mask."""
    f = first[xs]
    ok = f < big
    return h2[f[ok]], ok


def pairs_fanout(B, torch, device, rep, seed, mode, calls=6):
    """mode 'hops': a node's hop-1 row as a root against its hop-2 row as a child in ONE
    sample_fanout (call ids c and c + 1, same stream); 'auto': hop 2 of one call against
    hop 1 of the NEXT call under the graph's own call-id counter (c + 1 and c + 2: equal
    if the counter advanced by one per call instead of one per hop); 'multi': tile b hop 2
    against tile b + 1 hop 1 of one sample_fanout_multi (equal if tiles were one id apart)."""
    root_x, roots = _all_roots(torch, rep, device)
    out = {name: np.zeros((8, 8), np.int64) for name in PAIR_ROWS}
    B.set_seed(seed, PAIR_CALL + 100)
    prev = None
    for c in range(calls):
        if mode == "multi":
            res = B.sample_fanout_multi([roots] * 8, [[0], [0]], [8, 8], -1, call_id=PAIR_CALL + 200 + 16 * c)
        elif mode == "auto":
            res = [B.sample_fanout(roots, [[0], [0]], [8, 8], -1)]
        else:
            res = [B.sample_fanout(roots, [[0], [0]], [8, 8], -1, call_id=PAIR_CALL + 300 + 2 * c)]
        for nb, _, _ in res:
            _, _, _, first, h1, h2 = fanout_tables(torch, rep, root_x, nb, (8, 8))
            for name, (j, *per) in PAIR_ROWS.items():
                xs, _ = _row_roots(torch, rep, device, j)
                if mode == "hops":
                    # x as the child of ANOTHER root: whether x is found must not depend on
                    # x's own hop-1 row (it does where x lists itself)
                    par = h1.reshape(-1)
                    _, px = _decode(torch, rep, par, -1)
                    other = (par != -1) & (px != root_x.repeat_interleave(8))
                    ofirst, _ = _first_occurrence(torch, px, other, rep.n)
                    rows2, ok = _rows_of(torch, rep, ofirst, h1.numel(), h2, xs)
                    out[name] += _pair_table(torch, _cells(torch, rep, h1[xs][ok], per), _cells(torch, rep, rows2, per))
                elif prev is not None:
                    pfirst, pbig, ph2 = prev
                    rows2, ok = _rows_of(torch, rep, pfirst, pbig, ph2, xs)
                    out[name] += _pair_table(torch, _cells(torch, rep, rows2, per), _cells(torch, rep, h1[xs][ok], per))
            prev = (first, h1.numel(), h2)
        if mode == "multi":
            prev = None
    return {k: (t, int(t.sum())) for k, t in out.items()}


def pairs_walk(B, torch, device, rep, seed, calls=48):
    """The move from node x at step s against the move from x at step s + 1 (s even, so
    no draw is used twice), whoever stands there: call ids c + s and c + s + 1, same
    stream."""
    L = 8
    root_x, roots = _all_roots(torch, rep, device)
    n = roots.numel()
    out = {name: np.zeros((8, 8), np.int64) for name in PAIR_ROWS}
    B.set_seed(seed)
    step = torch.arange(L, dtype=torch.int64, device=device)[None, :]
    for c in range(calls):
        w = B.random_walk(roots, [[0]] * L, 1.0, 1.0, -1, call_id=PAIR_CALL + 1000 + L * c)
        cur, nxt = w[:, :-1].reshape(-1), w[:, 1:].reshape(-1)
        valid = cur != -1
        _, cx = _decode(torch, rep, cur, -1)
        key = (step * rep.n + cx.reshape(n, L)).reshape(-1)
        first, big = _first_occurrence(torch, key, valid, L * rep.n)
        # at step s + 1 take x only where a walker ARRIVED from another node: whether x is
        # occupied then must not depend on x's own move at step s (it does for a self-loop)
        wv = w[:, :-1]
        arrived = torch.ones_like(wv, dtype=torch.bool)
        arrived[:, 1:] = wv[:, 1:] != wv[:, :-1]
        afirst, _ = _first_occurrence(torch, key, valid & arrived.reshape(-1), L * rep.n)
        for name, (j, *per) in PAIR_ROWS.items():
            xs, _ = _row_roots(torch, rep, device, j)
            for s in range(0, L, 2):
                fa, fb = first[s * rep.n + xs], afirst[(s + 1) * rep.n + xs]
                ok = (fa < big) & (fb < big)
                out[name] += _pair_table(torch, _cells(torch, rep, nxt[fa[ok]], per),
                                         _cells(torch, rep, nxt[fb[ok]], per))
    return {k: (t, int(t.sum())) for k, t in out.items()}


DOMAIN_R, DOMAIN_COUNT = 2048, 64


def domain_graph_raw(R=DOMAIN_R):
    """Every row a uniform-8 row, ids 1 .. 16 R; every node of type 0 and weight 1."""
    rep = Replicas(uniform_motif(1), R, base=1)
    return rep, rep.raw()


def pairs_domains(B, torch, device, rep, seed):
    """Sample j of row i of sample_n_with_types (domain 1, stream i, draws 2 j | 2 j + 1 =
    column | coin of the alias method) against draw 2 j of sample_neighbor for the node of
    id i (domain 0, stream i), same seed and call id.  Equal weights make both an index
    computation on their uniform: node = floor(n u), entry = floor(8 u); the cells are
    floor(8 u) on both sides."""
    n = rep.n
    B.set_seed(seed)
    nodes = B.sample_n_with_types(DOMAIN_COUNT, [0] * (n + 1), call_id=PAIR_CALL + 2000)[1:]      # rows 1 .. n
    a = (nodes - 1) * 8 // n
    root_x, roots = _all_roots(torch, rep, device)                                                # ids 1 .. n
    nb = B.sample_neighbor(roots, [0], 2 * DOMAIN_COUNT, -1, call_id=PAIR_CALL + 2000)[0][:, 0::2]
    pos, _ = _decode(torch, rep, nb, -1)
    b = (pos - (root_x % rep.M)[:, None] - 1) % rep.M
    assert bool((b < 8).all()) and bool(((a >= 0) & (a < 8)).all())
    t = _pair_table(torch, a, b)
    return {"uniform8": (t, int(t.sum()))}


def judge_pairs(report, label, tables, min_n=PAIR_MIN_N):
    bad = []
    for name, (t, N) in tables.items():
        assert N >= min_n, "%s/%s: %d pairs, sized for %d" % (label, name, N, min_n)
        pm = pair_marginal(name)
        stat, df, pv = pair_independence(t, pm, pm, MIN_EXPECTED, N)
        report.add("%s/%s" % (label, name), stat, df, N, pv)
        if not pv >= LEVEL:
            bad.append("%s/%s" % (label, name))
    return bad


# ---- node / type / root / layer draws
def node_graph_raw():
    """Three copies of the plain motif (48 nodes, ids 1..48), node type = copy."""
    rep = replicas("plain", 3)
    return rep, rep.raw()


def _judge_flat(report, label, counts, p, N):
    stat, df, pv = gof(counts, p, MIN_EXPECTED, N)
    report.add(label, stat, df, N, pv)
    return [] if pv >= LEVEL else [label]


def run_node_case(B, torch, case, seed, report):
    B.set_seed(seed)
    ids = B.sample_node(case["count"], case["types"] if len(case["types"]) > 1 else case["types"][0],
                        call_id=case["call_id"])
    assert ids.numel() == case["count"] and int(ids.min()) >= 1 and int(ids.max()) <= 48
    counts = torch.bincount(ids - 1, minlength=48).cpu().numpy()
    return _judge_flat(report, case["name"], counts, node_sampler_model(NODE_TYPES, NODE_WEIGHTS, case["types"]),
                       case["count"])


def run_nwt_case(B, torch, device, seed, report, rows=NWT_ROWS):
    """sample_n_with_types: row i draws from the sampler of types[i] on stream i."""
    types = NWT_TYPES * (rows // len(NWT_TYPES))
    B.set_seed(seed)
    ids = B.sample_n_with_types(NWT_COUNT, types, call_id=NWT_CALL)
    assert tuple(ids.shape) == (rows, NWT_COUNT) and int(ids.min()) >= 1 and int(ids.max()) <= 48
    bad = []
    for k, t in enumerate(NWT_TYPES):
        counts = torch.bincount((ids[k::len(NWT_TYPES)] - 1).reshape(-1), minlength=48).cpu().numpy()
        bad += _judge_flat(report, "n_with_types/type%d" % t, counts,
                           node_sampler_model(NODE_TYPES, NODE_WEIGHTS, [t]), rows // len(NWT_TYPES) * NWT_COUNT)
    return bad


ROOT_WEIGHTS = np.asarray([[float(i + 1) for i in range(16)],
                           [0, 3, 0, 1, 2, 0, 0, 5, 1, 0, 4, 4, 0.25, 8, 1, 0]], np.float32)
ROOT_BATCH, ROOT_M, ROOT_CALL = 2 * 16384, 512, 3400          # N = 8.4 M per weight row


def root_model(k):
    w = ROOT_WEIGHTS[k].astype(np.float64)
    return w / w.sum()


def run_root_case(sample_root, torch, device, seed, report, batch=ROOT_BATCH):
    """sample_root: batch row b (its own stream) draws ROOT_M of its 16 roots by weight;
    rows alternate between the two weight vectors.  sample_root(roots, weights, m, call_id)."""
    roots = torch.arange(1, 17, dtype=torch.int64, device=device)[None, :].repeat(batch, 1)
    w = torch.as_tensor(ROOT_WEIGHTS, device=device).repeat(batch // 2, 1)
    out = sample_root(roots, w, ROOT_M, ROOT_CALL)
    assert tuple(out.shape) == (batch, ROOT_M) and int(out.min()) >= 1 and int(out.max()) <= 16
    bad = []
    for k in range(2):
        counts = torch.bincount((out[k::2] - 1).reshape(-1), minlength=16).cpu().numpy()
        bad += _judge_flat(report, "sample_root/weights%d" % k, counts, root_model(k), batch // 2 * ROOT_M)
    return bad


LAYER_REPEAT, LAYER_CALLS, LAYER_CALL = 16, 16, 3500
LAYER_TYPES = {"plain": [0], "typed": [0, 2]}


def run_layer_case(sample_layer, torch, device, rep, graph, seed, report, calls=LAYER_CALLS):
    """sample_layer: one neighbour per listed root, stream = the POSITION in the list, so
    a root listed LAYER_REPEAT times draws LAYER_REPEAT independent neighbours.
    sample_layer(roots, edge_types, call_id) -> ids [n]."""
    root_x, roots = _all_roots(torch, rep, device)
    root_x, roots = root_x.repeat(LAYER_REPEAT), roots.repeat(LAYER_REPEAT)
    t = np.zeros((rep.M, rep.M + 1), np.int64)
    for c in range(calls):
        ids = sample_layer(roots, LAYER_TYPES[graph], LAYER_CALL + c)
        t += tally(torch, rep, root_x, ids.reshape(-1, 1), -1)
    N = rep.R * LAYER_REPEAT * calls
    return judge_rows(report, "sample_layer_" + graph, t,
                      [rep.motif.model(j, LAYER_TYPES[graph]) for j in range(rep.M)], [N] * rep.M)


LOCAL_BATCH, LOCAL_M, LOCAL_CALL = 16384, 512, 3600
LOCAL_FUNCS = ("sqrt", "")


def local_layer_lists():
    """The candidates of one batch row: the full typed neighbour lists of two nodes (rows 0
    and 2 of the typed motif) plus a repeat of the first list's head, so that (id, type)
    pairs recur and their weights add."""
    m = motif_of("typed")
    lists = []
    for j in (0, 2):
        ids, w, t = [], [], []
        for ty in range(3):
            a, b = m.rows[j][ty]
            ids += [x + 1 for x in a]
            w += list(b)
            t += [ty] * len(a)
        lists.append((ids, w, t))
    ids, w, t = lists[1]
    lists[1] = (ids + lists[0][0][:3], w + [0.5, 0.5, 7.0], t + lists[0][2][:3])
    return lists


def local_layer_case(weight_func):
    """(flat ids, w, t, idx [2, 2], model {(id, type): p}) of one batch row (n = 2 nodes)."""
    lists = local_layer_lists()
    ids = np.asarray(lists[0][0] + lists[1][0], np.int64)
    w = np.asarray(lists[0][1] + lists[1][1], np.float32)
    t = np.asarray(lists[0][2] + lists[1][2], np.int32)
    n0 = len(lists[0][0])
    idx = np.asarray([[0, n0], [n0, len(ids)]], np.int32)
    return ids, w, t, idx, local_layer_model(ids, w, t, weight_func)


def run_local_layer_case(local_sample_layer, torch, device, weight_func, seed, report, batch=LOCAL_BATCH):
    """local_sample_layer(idx, ids, w, t, batch, n, m, weight_func, call_id) -> (ids, w, types)."""
    ids, w, t, idx, model = local_layer_case(weight_func)
    per = len(ids)
    off = (np.arange(batch, dtype=np.int64) * per)[:, None, None]
    idx_all = (idx[None, :, :] + off).astype(np.int32).reshape(-1, 2)
    oid, _, ot = local_sample_layer(torch.as_tensor(idx_all, device=device),
                                    torch.as_tensor(np.tile(ids, batch), device=device),
                                    torch.as_tensor(np.tile(w, batch), device=device),
                                    torch.as_tensor(np.tile(t, batch), device=device),
                                    batch, 2, LOCAL_M, weight_func, LOCAL_CALL)
    assert oid.numel() == batch * LOCAL_M
    key = oid.to(torch.int64) * 3 + ot.to(torch.int64)
    assert int(key.min()) >= 3 and int(key.max()) < 17 * 3
    counts = torch.bincount(key, minlength=17 * 3).cpu().numpy()
    p = np.zeros(17 * 3)
    for (i, ty), v in model.items():
        p[i * 3 + ty] = v
    return _judge_flat(report, "local_sample_layer/%s" % (weight_func or "identity"), counts, p, batch * LOCAL_M)


# ------------------------------------------------------------------ the power table
PAIR_TESTS = ("draws_even", "draws_odd", "calls", "seeds", "ids", "hops", "auto", "multi", "walk", "domains")


def power_table():
    """Every statistic of the GPU file as (label, p, N, {planted bias: q}): the exact
    distribution, the number of draws the case is sized for, and the biases it must reject.
    The host test draws from p and from every q with numpy's generator; the GPU test runs
    the same runners, which compute the same p and assert the same N (or more)."""
    out = []
    for case in NEIGHBOR_CASES:
        for r in case_rows(case):
            if r["p"] is not None:
                out.append((r["label"], r["p"], r["N"], planted_marginal(r["p"])))
    for case in NODE_CASES:
        p = node_sampler_model(NODE_TYPES, NODE_WEIGHTS, case["types"])
        out.append((case["name"], p, case["count"], planted_marginal(p)))
    for t in NWT_TYPES:
        p = node_sampler_model(NODE_TYPES, NODE_WEIGHTS, [t])
        out.append(("n_with_types/type%d" % t, p, NWT_ROWS // len(NWT_TYPES) * NWT_COUNT, planted_marginal(p)))
    _, _, ty, w = typed_edge_records()
    for t in (0, 2, -1):
        p = edge_model(ty, w, t)
        out.append(("sample_edge/type%d" % t, p, EDGE_COUNT, planted_marginal(p)))
    p = np.full(LABELS, 1.0 / LABELS)
    out.append(("sample_graph_label", p, LABEL_COUNT, planted_marginal(p)))
    for k in range(2):
        out.append(("sample_root/weights%d" % k, root_model(k), ROOT_BATCH // 2 * ROOT_M, planted_marginal(root_model(k))))
    for g, ts in LAYER_TYPES.items():
        m = motif_of(g)
        for j in range(m.M):
            p = m.model(j, ts)
            if p is not None:
                out.append(("sample_layer_%s/%s" % (g, m.names[j]), p, R_GPU * LAYER_REPEAT * LAYER_CALLS,
                            planted_marginal(p)))
    for f in LOCAL_FUNCS:
        model = local_layer_case(f)[4]
        p = np.asarray([model[k] for k in sorted(model)])
        out.append(("local_sample_layer/%s" % (f or "identity"), p, LOCAL_BATCH * LOCAL_M, planted_marginal(p)))
    for case in WALK_CASES:
        m = motif_of(case["graph"])
        for j in range(m.M):
            p = m.model(j, [0])
            if p is not None:
                n = (R_GPU if case["walkers"] == "all" else R_GPU // 4) * case["calls"]
                out.append(("%s/%s" % (case["name"], m.names[j]), p, n, planted_marginal(p)))
    for g in ("plain", "sorted"):
        m = motif_of(g)
        for p_, q_ in N2V_PQ:
            for name, prev, cur, model, sized in n2v_expected_rows(m, p_, q_, R_GPU * N2V_PER_NODE):
                if model is None:
                    continue
                planted = {v: n2v_model(m, prev, cur, p_, q_, first_step=prev is None, variant=v)
                           for v in ("swapped", "undivided")}
                out.append(("n2v_%s_p%g_q%g/%s" % (g, p_, q_, name), model, sized, planted))
    hub = motif_of("hub")
    for j in range(3):
        pc = hub_cells(hub, hub.model(j, [0]))[1]
        out.append(("hub_neighbor/" + hub.names[j], pc, R_HUB * HUB_COUNT * HUB_CALLS, planted_marginal(pc)))
    for g in ("hub", "hubsorted"):
        m = motif_of(g)
        for p_, q_ in N2V_PQ:
            for name, si, cur, model, sized in hub_n2v_rows(m, p_, q_, R_HUB * HUB_N2V_PER_NODE):
                cell, pc = hub_cells(m, model)
                planted = {}
                for v in ("swapped", "undivided"):
                    qm = n2v_model(m, si + 1, (si + 1) if cur is None else cur, p_, q_, first_step=cur is None, variant=v)
                    planted[v] = np.bincount(cell[:-1], weights=qm, minlength=len(pc))
                out.append(("n2v_%s_p%g_q%g/%s" % (g, p_, q_, name), pc, sized, planted))
    for test in PAIR_TESTS:
        for name in (PAIR_ROWS if test != "domains" else ("uniform8",)):
            pm = pair_marginal(name)
            out.append(("pair_%s/%s" % (test, name), np.outer(pm, pm).reshape(-1), PAIR_MIN_N,
                        {"repeat": planted_pair(pm, pm, PAIR_EPS).reshape(-1)}))
    return out


# ------------------------------------------------------------------ the hub motif
R_HUB = 64
HUB_BINS = 32
HUB_COUNT, HUB_CALLS, HUB_CALL = 256, 512, 70000            # N = 64 * 256 * 512 = 8.4 M per long row
HUB_N2V_PER_NODE, HUB_N2V_CALL = 2048, 71000


def hub_cells(motif, p):
    """Cells of a long row's distribution p [M]: the hub's 6 000 entries go into 32 bins of
    equal expected mass (in position order); other rows keep their positions (gof merges
    the light ones).  Returns (cell of every position [M + 1] with the default fill last,
    cell probabilities)."""
    if np.count_nonzero(p) > 2000:
        cell = np.zeros(motif.M + 1, np.int64)
        nz = p > 0
        cell[:-1][nz] = equal_mass_bins(p[nz], HUB_BINS)
        pc = np.bincount(cell[:-1][nz], weights=p[nz], minlength=HUB_BINS + 1)
        cell[:-1][~nz] = HUB_BINS                            # positions of probability 0 and the fill:
        cell[-1] = HUB_BINS                                  # one cell that must stay empty
        return cell, pc
    cell = np.arange(motif.M + 1)
    return cell, np.concatenate([p, [0.0]])


def run_hub_neighbor(B, torch, device, rep, seed, report, calls=HUB_CALLS):
    """sample_neighbor on the three long rows of every copy of the hub motif."""
    m, M = rep.motif, rep.M
    xs = torch.cat([_row_roots(torch, rep, device, j)[0] for j in range(3)])
    roots = rep.base + rep.stride * xs
    B.set_seed(seed)
    t = np.zeros((3, M + 1), np.int64)
    for c in range(calls):
        ids = B.sample_neighbor(roots, [0], HUB_COUNT, -1, call_id=HUB_CALL + c)[0]
        pos, x = _decode(torch, rep, ids, -1)
        assert bool((_copy_of(rep, x) == _copy_of(rep, xs)[:, None]).all())
        key = rep.pos_from_x(xs)[:, None] * (M + 1) + pos
        t += torch.bincount(key.reshape(-1), minlength=3 * (M + 1)).reshape(3, M + 1).cpu().numpy()
    bad, N = [], rep.R * HUB_COUNT * calls
    for j in range(3):
        cell, pc = hub_cells(m, m.model(j, [0]))
        bad += _judge_flat(report, "hub_neighbor/" + m.names[j], np.bincount(cell, weights=t[j]).astype(np.int64), pc, N)
    return bad


def hub_n2v_rows(motif, p, q, walkers_per_start_row):
    """[(label, start index, cur or None, model [M], sized N)]: step 1 from rows 1 and 2, step
    2 for the first moves onto the long rows 0, 1, 2 (first moves onto short rows are counted
    in step 1 only)."""
    rows = []
    for si, s in enumerate((1, 2)):
        p1 = n2v_model(motif, None, s, p, q, first_step=True)
        rows.append(("step1/%d" % s, si, None, p1, walkers_per_start_row))
        for cur in range(3):
            if p1[cur] > 0:
                rows.append(("step2/%d>%d" % (s, cur), si, cur, n2v_model(motif, s, cur, p, q),
                             lower_bound(walkers_per_start_row, p1[cur])))
    return rows


def run_hub_n2v(B, torch, device, rep, p, q, seed, report, label, per_node=HUB_N2V_PER_NODE):
    """node2vec on the hub motif: child lists of 600 and 6 000 entries against parent lists of
    600 (several 256-entry chunks of the kernels), walkers = streams."""
    m, M = rep.motif, rep.M
    starts = torch.cat([_row_roots(torch, rep, device, j)[1].repeat_interleave(per_node) for j in (1, 2)])
    B.set_seed(seed)
    w = B.random_walk(starts, [[0], [0]], p, q, -1, call_id=HUB_N2V_CALL)
    p0, x0 = _decode(torch, rep, w[:, 0], -1)
    p1, x1 = _decode(torch, rep, w[:, 1], -1)
    p2, x2 = _decode(torch, rep, w[:, 2], -1)
    assert bool((p1 < M).all()) and bool((p2 < M).all())
    assert bool((_copy_of(rep, x1) == _copy_of(rep, x0)).all()) and bool((_copy_of(rep, x2) == _copy_of(rep, x0)).all())
    si = p0 - 1
    t1 = torch.bincount(si * (M + 1) + p1, minlength=2 * (M + 1)).reshape(2, M + 1).cpu().numpy()
    onlong = p1 < 3
    t2 = torch.bincount(((si * 3 + p1) * (M + 1) + p2)[onlong], minlength=6 * (M + 1)).reshape(2, 3, M + 1).cpu().numpy()
    bad = []
    for name, s_i, cur, model, sized in hub_n2v_rows(m, p, q, rep.R * per_node):
        row = t1[s_i] if cur is None else t2[s_i, cur]
        N = int(row.sum())
        assert N >= sized, (label, name, N, sized)
        cell, pc = hub_cells(m, model)
        bad += _judge_flat(report, "%s/%s" % (label, name), np.bincount(cell, weights=row).astype(np.int64), pc, N)
    return bad
