"""Case builders for the neighbour-listing family (get_full_neighbor with both fill kernels,
neighbor_post_process, get_top_k_neighbor, idx_gather / data_gather), shared by
test_neighbor_lists_host.py (which proves from the oracle alone that the cases reach what
they claim to reach) and test_neighbor_lists_gpu.py (which runs them).  No GPU import.

The case graph is built from an explicit table of per-(node, type) degrees, so the row
totals the kernels see sit ON the branch boundaries instead of being met by chance:
64 / 65 (a wave ranks a row / segmented radix sort and the long-row top-k branches),
256 (one window of the balanced fill), 2049 (more than one window's worth in one row).

Every raw weight is a small integer, so the float32 running sums of a row are exact and the
weight an entry reports (a difference of two running sums) is the raw weight: a family such
as "strictly ascending" is a property of what the kernels read, not only of what was fed in."""
import numpy as np

TOTALS = (0, 1, 3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 2049)
TYPE_LISTS = ([0], [1], [0, 1], [1, 0], [1, 1])
TOP_KS = (1, 2, 7, 8, 9, 63, 64, 65, 300)
LIMITS = (None, 0, 1, 2, 63, 64, 65, 5000)
FAMILIES = ("asc", "desc", "equal", "five", "zeros", "tail9", "shared")
# (type 0, type 1) degrees every family gets: every type list above then has a row of the
# family with a total of at most 64, one of 65..256 and one over 256; (40, 41): a row of at
# most 64 entries per type and more than 64 over both
CLASS_PAIRS = ((20, 30), (40, 41), (100, 90), (300, 400))

SUPER_THRESHOLD = 32 << 20      # FullNbFillBalancedKernel: calls with this many entries take 8 windows a search
WINDOW = 256                    # entries per wave-step of the balanced fill
SUPER = 8 * WINDOW


def _cat(*parts):
    """Concatenate as uint64 (numpy would promote a mix of int64 and uint64 to float64)."""
    return np.concatenate([np.asarray(p, np.uint64).reshape(-1) for p in parts])


def list_total(d0, d1, et):
    """Entries of a row with degrees (d0, d1) under type list et (unknown types list nothing)."""
    return sum((d0, d1)[t] for t in et if 0 <= t < 2)


def doubled_totals(s):
    """[1, 1] lists type 1's segment twice: only even totals exist.  An odd member of TOTALS
    is stood in for by its two even neighbours."""
    return (s,) if s % 2 == 0 else (s - 1, s + 1)


def degree_table():
    """[(d0, d1, family)] in a fixed order; families go round the table, the rows of
    CLASS_PAIRS name theirs."""
    rows = []

    def add(d0, d1, fam=None):
        rows.append((int(d0), int(d1), fam if fam is not None else FAMILIES[len(rows) % len(FAMILIES)]))

    for s in TOTALS:                      # [0] (and the pair lists with one segment empty)
        add(s, 0)
    for s in TOTALS:                      # [1]
        add(0, s)
    for s in TOTALS:                      # [0, 1] / [1, 0]: both segments present
        if s >= 3:
            add(s // 3, s - s // 3)
            add(s - 1, 1)
            add(1, s - 1)
    for s in TOTALS:                      # [1, 1]
        for e in doubled_totals(s):
            add(3, e // 2)
    for d0 in range(9):                   # short rows of every small shape
        for d1 in (0, 1, 2, 7):
            add(d0, d1)
    for k in TOP_KS:                      # a total equal to every k, one and two segments
        add(k, 0)
        add(0, k)
        if k >= 2:
            add(k // 2, k - k // 2)
    for fam in FAMILIES:
        for d0, d1 in CLASS_PAIRS:
            add(d0, d0 if fam == "shared" else d1, fam)
    return rows


def _segment_weights(fam, d0, d1):
    """Raw weights of one row, type 0's segment then type 1's (storage order)."""
    L = d0 + d1
    p = np.arange(L)
    j = np.concatenate([np.arange(d0), np.arange(d1)])           # position inside its segment
    t = np.concatenate([np.zeros(d0, np.int64), np.ones(d1, np.int64)])
    if fam == "asc":
        w = p + 1
    elif fam == "desc":
        w = L - p
    elif fam == "equal":
        w = np.full(L, 2)
    elif fam == "five":
        w = 1 + (p * 7) % 5
    elif fam == "zeros":
        w = np.where(p % 2 == 0, 0, 1 + p % 3)
    elif fam == "tail9":
        # the last 9 entries of a segment are its heaviest, type 1's heavier than type 0's:
        # the last 9 of the row are the row's heaviest
        seg_len = np.where(t == 0, d0, d1)
        tail = j >= seg_len - 9
        w = np.where(tail, 100 * (t + 1) + j - (seg_len - 9), 1 + j % 4)
    elif fam == "shared":
        # the same values at the same positions of both segments: which of two equal weights
        # comes first is decided by the LISTED order of the types
        w = 1 + (j * 3) % 5
    else:
        raise ValueError(fam)
    return w.astype(np.float32)


class CaseGraph:
    """Raw adjacency of the case graph + what the tests ask of it."""

    def __init__(self):
        table = degree_table()
        n = len(table)
        # spread the table over the id space: a multiplier coprime to n
        step = next(s for s in range(89, 200) if np.gcd(s, n) == 1)
        table = [table[(i * step) % n] for i in range(n)]
        self.table = table
        n_big = 12
        small = 1 + 37 * np.arange(n - 40 - n_big, dtype=np.uint64)
        mid = np.uint64(10 ** 12) + np.uint64(1009) * np.arange(40, dtype=np.uint64)
        big = np.array([2 ** 63, 2 ** 63 + 1, 2 ** 63 + 2, 2 ** 63 + 2 ** 31, 2 ** 63 + 2 ** 32 + 7,
                        2 ** 63 + 2 ** 40, 2 ** 63 + 2 ** 62, 2 ** 64 - 2 ** 33, 2 ** 64 - 2 ** 32,
                        2 ** 64 - 4, 2 ** 64 - 3, 2 ** 64 - 2], np.uint64)
        self.ids = np.concatenate([small, mid, big])
        assert len(self.ids) == n and np.all(self.ids[1:] > self.ids[:-1])
        self.deg = np.array([(a, b) for a, b, _ in table], np.int64)
        self.family = [f for _, _, f in table]
        self.seg = np.zeros(2 * n + 1, np.int64)
        self.seg[1:] = np.cumsum(self.deg.reshape(-1))
        E = int(self.seg[-1])
        # ids that are nobody's row: small, between two rows, at and above 2^63, the largest key
        self.no_row = np.array([2, 10 ** 12 + 1, 2 ** 63 + 3, 2 ** 64 - 5, 2 ** 64 - 1], np.uint64)
        rng = np.random.default_rng(2049)
        pool = np.concatenate([self.ids, self.no_row, big, big])       # (the large ids drawn more often)
        self.nbr = rng.choice(pool, E).astype(np.uint64)
        w = np.zeros(E, np.float32)
        for r in range(n):
            b, e = int(self.seg[2 * r]), int(self.seg[2 * r + 2])
            w[b:e] = _segment_weights(self.family[r], *self.deg[r])
            if e - b >= 2:
                self.nbr[e - 1] = self.nbr[b]          # a duplicate key in every row of two or more
        self.w = w
        self.unknown = np.array([4, 2 ** 63 + 5], np.uint64)

    def csr(self, O):
        return O.csr_from_raw(self.ids, self.seg, self.nbr, self.w, 2)

    def rows_with(self, d0, d1):
        return [i for i in range(len(self.ids)) if tuple(self.deg[i]) == (d0, d1)]

    def totals(self, et):
        return np.array([list_total(a, b, et) for a, b in self.deg], np.int64)

    def queries(self):
        """An empty row first, every node, id 0, two unknown ids, repeated ids (the longest row
        back to back among them), an empty row last (the balanced fill reads the call's total
        from the last query's idx)."""
        empty = self.ids[self.rows_with(0, 0)]
        longest = self.ids[self.rows_with(2049, 0)[0]]
        rep = np.array([self.ids[3], self.ids[3], longest, longest, self.ids[-1], self.ids[-1],
                        self.ids[-1]], np.uint64)
        return _cat(empty[:1], self.ids, [0], self.unknown, rep, self.ids[::5],
                    self.unknown[:1], empty[-1:])

    def batches(self, et):
        """Post-process batches by row length under et: no row over 64 (the library pass is
        skipped), only rows over 64 (nothing for the wave-rank kernel), and everything."""
        tot = self.totals(et)
        short = _cat(self.ids[tot <= 64], [0], self.unknown)
        long_ = self.ids[tot > 64]
        return {"short": short, "long": long_, "mixed": self.queries()}


def as_i64(a):
    """uint64 ids as the int64 the Python surface takes (same bits)."""
    return np.ascontiguousarray(np.asarray(a, np.uint64)).view(np.int64)


# ----------------------------------------------------------------------------------------
# The graph of the super-window path: a few hubs, rows of 300..2000, rows of 0..8 entries,
# about 2 M edges; a query list whose result is just over SUPER_THRESHOLD entries.
# ----------------------------------------------------------------------------------------
HUBS = ((2 ** 20 + 3, 5), (300001, 0), (70001, 2))      # (type 0, type 1) degrees
HUB_ENTRIES = 2 ** 20 + 3                               # of hub 0 under [0]
N_MEDIUM, N_SHORT = 300, 600


class SuperGraph:
    def __init__(self):
        rng = np.random.default_rng(33554432)
        med = np.stack([rng.integers(150, 1000, N_MEDIUM), rng.integers(150, 1000, N_MEDIUM)], axis=1)
        short = np.stack([rng.integers(0, 5, N_SHORT), rng.integers(0, 5, N_SHORT)], axis=1)
        short[::7] = 0                                          # rows without any entry
        self.deg = np.concatenate([np.array(HUBS, np.int64), med, short]).astype(np.int64)
        n = len(self.deg)
        self.ids = (np.uint64(5) + np.uint64(3) * np.arange(n, dtype=np.uint64))
        self.ids[-20:] += np.uint64(2 ** 63)                    # some rows at and above 2^63
        self.hub = self.ids[:3]
        self.medium = self.ids[3:3 + N_MEDIUM]
        self.short = self.ids[3 + N_MEDIUM:]
        self.empty = self.short[::7]
        self.seg = np.zeros(2 * n + 1, np.int64)
        self.seg[1:] = np.cumsum(self.deg.reshape(-1))
        E = int(self.seg[-1])
        self.n_edges = E
        self.nbr = rng.choice(self.ids, E).astype(np.uint64)
        self.w = (rng.integers(0, 64, E) * 0.125).astype(np.float32)     # zeros among them
        self.unknown = np.array([1, 2, 4, 2 ** 63 + 1], np.uint64)

    def csr(self, O):
        return O.csr_from_raw(self.ids, self.seg, self.nbr, self.w, 2)

    def queries(self):
        """Type list [0, 1].  In order: empty rows and unknown ids; the largest hub back to
        back (whole super windows inside one row); a long run of short and empty rows and
        unknown ids (super windows of many rows); the medium rows over and over (a 256-entry
        window inside one row, its super window over several); the other hubs with empty rows
        and unknown ids on both sides; empty rows and unknown ids last."""
        h0, h1, h2 = self.hub
        gap = np.array([self.empty[0], self.unknown[0], self.empty[1], self.unknown[3]], np.uint64)
        many = _cat(self.short, self.unknown, self.short[::-1], self.unknown, self.short,
                    self.short[::3])
        q = _cat(gap, np.repeat(h0, 12), gap, many, np.tile(self.medium, 18), gap,
                 np.tile(_cat([h1], gap, [h2, h2]), 10), many[:997], np.repeat(h0, 10), gap,
                 np.tile(_cat([h2], gap[:2]), 20))
        tot = dict(zip(self.ids.tolist(), self.deg.sum(1).tolist()))
        total = sum(tot.get(int(x), 0) for x in q)
        if total % WINDOW == 0:                                   # the last window is a partial one
            q = _cat(q, self.short[self.deg[3 + N_MEDIUM:].sum(1) == 1][:1])
        return _cat(q, gap)


def window_rows(idx, span):
    """(first row, last row) of every window of `span` entries of a result with row bounds
    idx [n, 2], as the balanced fill finds them: the first row whose end exceeds the entry."""
    ends = np.asarray(idx)[:, 1].astype(np.int64)
    total = int(ends[-1])
    w0 = np.arange(0, total, span, dtype=np.int64)
    w1 = np.minimum(w0 + span, total) - 1
    return np.searchsorted(ends, w0, side="right"), np.searchsorted(ends, w1, side="right")
