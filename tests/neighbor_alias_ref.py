"""numpy restatement of the alias neighbour mode (euler_amd/csrc/nb_alias.h, nb_alias_draw.h): the
build of the tables - AliasMethod::Init over FastWeightedCollection's normalised weights, plus the
zero-weight fix-up - and the draw with the output conventions of sample_neighbor / sample_fanout.
Written from the documented rules, not from the kernels; the uniforms come from
oracle.uniform_at and the type draw from oracle.random_select."""
import math

import numpy as np

F = np.float32
U = 2.0 ** -24


# ------------------------------------------------------------------ build
def row_weights(prefix_w_row):
    """w_i = fl(prefix_w[i] - prefix_w[i - 1]) over a WHOLE row, 0 before its first edge."""
    pw = np.asarray(prefix_w_row, F)
    return (pw - np.concatenate([np.zeros(1, F), pw[:-1]])).astype(F)


def normalise(w):
    """(S, norm): the sequential f32 sum and fl(w_i / S) (FastWeightedCollection::Init)."""
    w = np.asarray(w, F)
    S = F(0)
    for x in w:
        S = F(S + x)
    return S, (w / S).astype(F) if S != 0 else np.zeros(len(w), F)


def alias_init(norm):
    """AliasMethod::Init (alias_method.cc:23-63): LIFO stacks, avg in double, working weights in
    float, prob = fl(w[less] * n).  -> (prob f32, alias int64)."""
    w = np.asarray(norm, F).copy()
    n = len(w)
    prob, alias = np.zeros(n, F), np.zeros(n, np.int64)
    avg = 1.0 / float(n)
    small, large = [], []
    for i in range(n):
        (large if float(w[i]) > avg else small).append(i)
    fn = F(n)
    while large and small:
        less, more = small.pop(), large.pop()
        prob[less] = F(w[less] * fn)
        alias[less] = more
        w[more] = F(float(F(w[more] + w[less])) - avg)
        (large if float(w[more]) > avg else small).append(more)
    for i in small + large:
        prob[i] = F(1.0)
    return prob, alias


def fixup(w, prob, alias):
    """An entry of weight 0 that left the build with prob != 0 gets prob 0 and the FIRST entry of
    the largest weight as its alias.  In place; returns the indices it changed."""
    w = np.asarray(w, F)
    changed = [i for i in range(len(w)) if w[i] == 0 and prob[i] != 0]
    for i in changed:
        prob[i] = F(0)
        alias[i] = int(np.argmax(w))
    return changed


def build_group(w):
    """(prob, alias, changed) of one group's weights, or None when the group has no table."""
    w = np.asarray(w, F)
    S, norm = normalise(w)
    if len(w) == 0 or S == 0:
        return None
    prob, alias = alias_init(norm)
    return prob, alias, fixup(w, prob, alias)


def table_mass(prob, alias):
    """q_i = (prob_i + sum over alias_j == i of (1 - prob_j)) / d in float64: what the table draws."""
    d = len(prob)
    p = np.asarray(prob, np.float64)
    return (p + np.bincount(alias, weights=1.0 - p, minlength=d)) / d


def mass_bound(d):
    """|q_i - w_i / sum(w)| <= this, from the count of f32 roundings in the build (u = 2^-24).
    norm_i = p_i (1 + delta), |delta| <= g := gamma(d + 1): d - 1 adds of S, one division, slack;
    so sum(norm) = 1 + eps, |eps| <= g.  An iteration of the build makes three f32 roundings - the
    add and the store of the working weight of `more`, the product of prob - each on a value <= 1 +
    g (working weights only shrink); there are at most d iterations: R := 3 d u (1 + g) in all.  An
    entry finished inside the loop is off by its own share of R.  The drained entries get prob 1,
    that is 1 / d instead of their working weight; only one stack drains more than its rounding,
    so those errors share a sign and each is at most their sum, which is - eps less the loop's
    roundings (the table's mass is exactly 1): B := g + R.  The fix-up moves at most that sum once
    more onto the heaviest entry: 2 B.  Last, |norm_i - p_i| <= g."""
    g = (d + 1) * U / (1 - (d + 1) * U)
    return 2 * (g + 3 * d * U * (1 + g)) + g


class Tables:
    """The entries of every row of a CSR (oracle.CSR fields), at the edges' flat indices."""

    def __init__(self, csr):
        T = csr.n_types
        E = len(csr.nbr)
        self.csr, self.T = csr, T
        self.id_self = csr.nbr.astype(np.uint64).copy()
        self.id_alias = np.zeros(E, np.uint64)
        self.prob, self.w_self, self.w_alias = np.zeros(E, F), np.zeros(E, F), np.zeros(E, F)
        self.has_table = np.zeros(csr.n_rows * T, bool)
        self.changed = []                       # flat indices the fix-up changed
        self.alias_idx = np.zeros(E, np.int64)  # within the group
        for r in range(csr.n_rows):
            b0, e0 = int(csr.row_ptr[r]), int(csr.row_ptr[r + 1])
            w = row_weights(csr.prefix_w[b0:e0])
            te = csr.type_end[r * T:(r + 1) * T]
            for t in range(T):
                b, e = (0 if t == 0 else int(te[t - 1])), int(te[t])
                res = build_group(w[b:e]) if e > b else None
                if res is None:
                    self.id_self[b0 + b:b0 + e] = 0
                    continue
                prob, alias, changed = res
                self.has_table[r * T + t] = True
                s = slice(b0 + b, b0 + e)
                self.prob[s], self.alias_idx[s] = prob, alias
                self.w_self[s], self.w_alias[s] = w[b:e], w[b:e][alias]
                self.id_alias[s] = csr.nbr[b0 + b:b0 + e][alias]
                self.changed += [b0 + b + i for i in changed]
        self.row_of = {int(i): r for r, i in enumerate(csr.row_id)}
        self.has_zero_nbr = bool((csr.nbr == 0).any())

    def rows(self, ids):
        """The export: (row_ptr, id_self, id_alias, prob, w_self, w_alias) of the listed rows."""
        sel, ptr = [], [0]
        for i in ids:
            r = self.row_of.get(int(i))
            if r is not None:
                sel += list(range(int(self.csr.row_ptr[r]), int(self.csr.row_ptr[r + 1])))
            ptr.append(len(sel))
        sel = np.asarray(sel, np.int64)
        return (np.asarray(ptr, np.int64), self.id_self[sel], self.id_alias[sel], self.prob[sel], self.w_self[sel],
                self.w_alias[sel])


# ------------------------------------------------------------------ draw
def _root(tab, node, edge_types, k):
    """None (a row without samples) or what its samples share."""
    csr, T = tab.csr, tab.T
    r = tab.row_of.get(int(node))
    if r is None:
        return None
    te = csr.type_end[r * T:(r + 1) * T]
    tp = csr.type_prefix[r * T:(r + 1) * T]
    if k == 1:
        t = int(edge_types[0])
        if t < 0 or t >= T:
            return None
        b, e = (0 if t == 0 else int(te[t - 1])), int(te[t])
        return None if e <= b else ("single", r, te, None)
    if 1 < k < T:
        if any(t < 0 or t >= T for t in edge_types):
            return None
        sub, s = [], F(0)
        for t in edge_types:
            s = F(s + F(tp[t] - (tp[t - 1] if t > 0 else F(0))))
            sub.append(s)
        return None if sub[-1] == 0 else ("sub", r, te, np.asarray(sub, F))
    return None if tp[T - 1] == 0 else ("all", r, te, np.asarray(tp, F))


def _sample(tab, O, root, edge_types, seed, call_id, node, j):
    mode, r, te, sums = root
    if mode == "single":
        t = int(edge_types[0])
    else:
        u = O.uniform_at(seed, call_id, 0, int(node), 4 * j)
        x = O.random_select(sums, 0, len(sums) - 1, u)
        t = int(edge_types[x]) if mode == "sub" else int(x)
    b, e = (0 if t == 0 else int(te[t - 1])), int(te[t])
    d = e - b
    ident, w = 0, F(0)
    if d > 0:
        u_col = O.uniform_at(seed, call_id, 0, int(node), 4 * j + 2)
        u_coin = O.uniform_at(seed, call_id, 0, int(node), 4 * j + 3)
        x = int(tab.csr.row_ptr[r]) + b + int(math.floor(float(d) * u_col))
        if u_coin < float(tab.prob[x]):
            ident, w = int(tab.id_self[x]), tab.w_self[x]
        else:
            ident, w = int(tab.id_alias[x]), tab.w_alias[x]
    if w == 0:                  # a group without a table: the sentinel
        ident, t = 0, 0
    return ident, F(w), t


def sample_neighbor(tab, O, seed, call_id, nodes, edge_types, count, layout="tf", default_node=-1,
                    root_mask=None, root_group=1):
    """-> (ids uint64 [n, count], weights f32, types int32, row mask uint8 [n])."""
    nodes = np.asarray(nodes).astype(np.uint64).reshape(-1)
    n, k, tf = len(nodes), len(edge_types), layout == "tf"
    ids, w, t = np.zeros((n, count), np.uint64), np.zeros((n, count), F), np.zeros((n, count), np.int32)
    mask = np.zeros(n, np.uint8)
    fill = (np.uint64(default_node & 0xFFFFFFFFFFFFFFFF), F(0), -1) if tf else (np.uint64(0), F(0), 0)
    memo = {}
    for i in range(n):
        node = 0 if root_mask is not None and root_mask[i // root_group] else int(nodes[i])
        if node not in memo:
            root = _root(tab, node, edge_types, k)
            row = None
            if root is not None:
                row = [_sample(tab, O, root, edge_types, seed, call_id, node, j) for j in range(count)]
                if tf and count > 0:
                    # the first-id-0 rule: slot 0 drops the row when its id is 0; another slot looks at
                    # slot 0 on graphs with a neighbour id 0, or when it drew the sentinel itself
                    first0 = row[0][0] == 0
                    row = [None if first0 and (j == 0 or tab.has_zero_nbr or row[j][1] == 0) else row[j]
                           for j in range(count)]
            memo[node] = row
        row = memo[node]
        for j in range(count):
            ids[i, j], w[i, j], t[i, j] = fill if row is None or row[j] is None else row[j]
        if count > 0:
            mask[i] = 1 if row is None or row[0] is None else 0
    return ids, w, t, mask


def sample_fanout(tab, O, seed, call_id, nodes, edge_types, counts, default_node=-1):
    """Hop h: call_id + h, on hop h - 1's TF-layout ids; the rows under a default row of hop h - 1
    sample as node id 0.  -> per hop (ids, weights, types) flattened."""
    roots = np.asarray(nodes).astype(np.uint64).reshape(-1)
    mask, group, out = None, 1, []
    for h, c in enumerate(counts):
        ids, w, t, m = sample_neighbor(tab, O, seed, call_id + h, roots, edge_types[h], c, "tf", default_node, mask,
                                       group)
        out.append((ids.reshape(-1), w.reshape(-1), t.reshape(-1)))
        roots, mask, group = ids.reshape(-1), m, c
    return out
