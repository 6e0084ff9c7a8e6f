"""Plain-torch reference of block construction (tf.unique in first-occurrence order, then the
res_n_id / edge_index arithmetic of UniqueDataFlow.produce_subgraph, neighbor_dataflow.py:84-110
of the reference project) and the comparison helper of tests/test_dataflow_blocks_gpu.py.

Nothing here comes from euler_amd; every function runs on whatever device its inputs are on.
Ids are int64 and are only ever compared for equality, so ids with bit 63 set (-1 = the all-ones
id among them) need no special case."""
import torch

NAMES = ("new_n_id", "res_n_id", "edge_src", "edge_dst", "e_type")


def _arange(n, like):
    return torch.arange(n, dtype=torch.int64, device=like.device)


def first_occurrence(v):
    """tf.unique / ID_UNIQUE: (the distinct values of v in the order of their first occurrence,
    for every element of v the index of its value in that list)."""
    v = v.reshape(-1)
    n = v.numel()
    if n == 0:
        return v.clone(), torch.empty(0, dtype=torch.int64, device=v.device)
    vals, inv_sorted = torch.unique(v, return_inverse=True)           # vals ascending
    first = torch.full((vals.numel(),), n, dtype=torch.int64, device=v.device)
    first.scatter_reduce_(0, inv_sorted, _arange(n, v), "amin")       # first position of each value
    order = torch.argsort(first)                                      # first positions are distinct
    rank = torch.empty_like(order)
    rank[order] = _arange(order.numel(), v)
    return vals[order], rank[inv_sorted]


def sage_block(nb, n_id, count, self_loops):
    """One hop over V = [nb | n_id], nb = `count` sampled neighbours of every node of n_id in row
    order: (new_n_id, res_n_id, edge_src, edge_dst)."""
    nb, n_id = nb.reshape(-1), n_id.reshape(-1)
    assert nb.numel() == n_id.numel() * count
    src = _arange(nb.numel(), nb) // count
    return full_block(nb, src, n_id, self_loops)


def full_block(nb, nb_src, n_id, self_loops):
    """The same for rows of different lengths: nb_src[e] = the index into n_id of the node that
    entry e of nb is a neighbour of."""
    nb, n_id = nb.reshape(-1), n_id.reshape(-1)
    new_n_id, inv = first_occurrence(torch.cat([nb, n_id]))
    res_n_id = inv[nb.numel():]
    edge_src = nb_src.reshape(-1).to(torch.int64)
    if self_loops:
        edge_src = torch.cat([edge_src, _arange(n_id.numel(), n_id)])
        edge_dst = inv
    else:
        edge_dst = inv[:nb.numel()]
    return new_n_id, res_n_id, edge_src, edge_dst


def nb_src_of_idx(idx):
    """The source of every neighbour from the [n, 2] (begin, end) array of get_full_neighbor."""
    lens = (idx[:, 1] - idx[:, 0]).to(torch.int64)
    return torch.repeat_interleave(_arange(idx.shape[0], idx), lens)


def _offsets(lens):
    return torch.cumsum(lens, 0) - lens


def sage_block_batched(nb, n_id, n_len, count, self_loops):
    """sage_block of M minibatches with ONE first_occurrence.  n_id holds the minibatches' layers
    one behind the other (minibatch b: n_len[b] ids), nb their neighbours in the same order
    (minibatch b: n_len[b] * count).  Returns (new_n_id, new_len, res_n_id, edge_src, edge_dst),
    every array the per-minibatch results one behind the other, new_len [M] the new layers'
    sizes.  Every position of V is tagged with its minibatch; the pairs (minibatch, id) go through
    first_occurrence as one number, minibatch * (number of distinct ids) + the id's code."""
    nb, n_id, n_len = nb.reshape(-1), n_id.reshape(-1), n_len.reshape(-1).to(torch.int64)
    M = n_len.numel()
    assert n_id.numel() == int(n_len.sum()) and nb.numel() == n_id.numel() * count
    mbs = _arange(M, n_id)
    tag_n = torch.repeat_interleave(mbs, n_len)
    tag_nb = torch.repeat_interleave(mbs, n_len * count)
    loc_n = _arange(n_id.numel(), n_id) - _offsets(n_len)[tag_n]                # index inside the minibatch
    loc_nb = _arange(nb.numel(), n_id) - _offsets(n_len * count)[tag_nb]
    v_off = _offsets(n_len * (count + 1))                                       # V of minibatch b starts here
    at_nb = v_off[tag_nb] + loc_nb
    at_n = v_off[tag_n] + n_len[tag_n] * count + loc_n
    total = nb.numel() + n_id.numel()
    V = torch.empty(total, dtype=torch.int64, device=n_id.device)
    tag = torch.empty(total, dtype=torch.int64, device=n_id.device)
    V[at_nb], V[at_n] = nb, n_id
    tag[at_nb], tag[at_n] = tag_nb, tag_n
    vals, code = torch.unique(V, return_inverse=True)
    K = max(int(vals.numel()), 1)
    assert M * K < 2 ** 62
    keys, inv = first_occurrence(tag * K + code)
    # the positions are in minibatch order, so the distinct pairs are too
    new_tag = keys // K
    new_n_id = vals[keys % K] if vals.numel() else V.clone()
    new_len = torch.bincount(new_tag, minlength=M)
    inv = inv - _offsets(new_len)[tag]
    res_n_id = inv[at_n]
    if self_loops:
        edge_src = torch.empty(total, dtype=torch.int64, device=n_id.device)
        edge_src[at_nb], edge_src[at_n] = loc_nb // count, loc_n
        edge_dst = inv
    else:
        edge_src, edge_dst = loc_nb // count, inv[at_nb]
    return new_n_id, new_len, res_n_id, edge_src, edge_dst


def ragged(padded, lens):
    """The rows' valid prefixes of a padded [M, cap] tensor, one behind the other."""
    lens = lens.reshape(-1).to(device=padded.device, dtype=torch.int64)
    mask = _arange(padded.shape[1], padded)[None, :] < lens[:, None]
    return padded[mask]


def valid_prefix(padded, counts, fanouts, self_loops):
    """Blocks padded to the worst case (sync=False) + their counts -> the blocks a synchronous call
    returns.  padded[h] = (n_id, res_n_id, edge_src, edge_dst, ...)."""
    cnt = [int(c) for c in counts.reshape(-1).tolist()]
    out = []
    for h, blk in enumerate(padded):
        e = cnt[h] * int(fanouts[h]) + (cnt[h] if self_loops else 0)
        out.append((blk[0][:cnt[h + 1]], blk[1][:cnt[h]], blk[2][:e], blk[3][:e]))
    return out, cnt


def _first_diff(a, b):
    if a.shape != b.shape:
        return "shapes %s / %s" % (tuple(a.shape), tuple(b.shape))
    at = int(torch.nonzero(a != b)[0, 0])
    return "first at %d: %d / %d (%d differ)" % (at, int(a[at]), int(b[at]), int((a != b).sum()))


def compare_blocks(got, got_counts, want, what=""):
    """Exact equality of every array of every hop and of the layer sizes; AssertionError names
    the first array that differs.  got[h] / want[h] = (new_n_id, res_n_id, edge_src, edge_dst
    [, e_type]) at their valid lengths; want comes from sage_block / full_block, got_counts =
    the layer sizes the code under test reports ([layers + 1])."""
    want_counts = [int(want[0][1].numel())] + [int(w[0].numel()) for w in want]
    assert [int(c) for c in got_counts] == want_counts, \
        "%s: layer sizes %s, reference %s" % (what, [int(c) for c in got_counts], want_counts)
    assert len(got) == len(want), "%s: %d blocks, reference %d" % (what, len(got), len(want))
    for h, (g, w) in enumerate(zip(got, want)):
        for x in range(len(w)):
            if w[x] is None:
                continue
            a, b = g[x].reshape(-1).to(torch.int64), w[x].reshape(-1).to(torch.int64)
            assert a.device == b.device, "%s: hop %d %s on %s, reference on %s" % (what, h, NAMES[x], a.device, b.device)
            if not torch.equal(a, b):
                raise AssertionError("%s: hop %d %s differs, %s" % (what, h, NAMES[x], _first_diff(a, b)))


def compare_batched(got, got_counts, want, what=""):
    """The same for M minibatches in the batched form: got[h] = (new_n_id, res_n_id, edge_src,
    edge_dst) with the minibatches' valid prefixes one behind the other (ragged), got_counts
    [M, layers + 1]; want[h] = what sage_block_batched returned for hop h, want_n0 [M]."""
    gc = got_counts.to(torch.int64)
    for h, w in enumerate(want):
        new_len = w[1].to(gc.device)
        if not torch.equal(gc[:, h + 1], new_len):
            raise AssertionError("%s: sizes of layer %d differ, %s" % (what, h + 1, _first_diff(gc[:, h + 1], new_len)))
        for x, y in enumerate((w[0], w[2], w[3], w[4])):
            a = got[h][x].reshape(-1)
            if not torch.equal(a, y):
                raise AssertionError("%s: hop %d %s differs, %s" % (what, h, NAMES[x], _first_diff(a, y)))
