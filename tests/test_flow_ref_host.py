"""CPU-only: the reference of tests/flow_ref.py against a literal loop and the oracle's ID_UNIQUE,
its batched form against the per-minibatch loop, and the comparison helper of
tests/test_dataflow_blocks_gpu.py against correct results with one planted fault each."""
import numpy as np
import pytest
import torch

import flow_ref as FR


def loop_unique(v):
    """first-occurrence unique as a dictionary of first positions"""
    seen, uniq, inv = {}, [], []
    for x in v:
        if x not in seen:
            seen[x] = len(uniq)
            uniq.append(x)
        inv.append(seen[x])
    return uniq, inv


def loop_block(nb, n_id, count, self_loops):
    uniq, inv = loop_unique(list(nb) + list(n_id))
    src = [i // count for i in range(len(nb))]
    if self_loops:
        return uniq, inv[len(nb):], src + list(range(len(n_id))), inv
    return uniq, inv[len(nb):], src, inv[:len(nb)]


def id_vectors():
    rng = np.random.default_rng(11)
    hashed = rng.integers(-2 ** 63, 2 ** 63 - 1, 40, dtype=np.int64)
    out = {
        "empty": np.zeros(0, np.int64),
        "one": np.array([7], np.int64),
        "all_equal": np.full(300, -1, np.int64),
        "all_distinct": rng.permutation(5000).astype(np.int64) - 2500,
        "small_pool": rng.integers(-3, 4, 4097),
        "hashed_pool": rng.choice(np.concatenate([hashed, [-1, 0, 2 ** 63 - 1, -2 ** 63]]), 3000),
        "side_first": np.concatenate([[-1], rng.integers(0, 50, 1500), [-1, 0]]),
    }
    return {k: v.astype(np.int64) for k, v in out.items()}


@pytest.mark.parametrize("name", sorted(id_vectors()))
def test_first_occurrence_vs_loop_and_oracle(O, name):
    v = id_vectors()[name]
    uniq, inv = FR.first_occurrence(torch.as_tensor(v))
    lu, li = loop_unique(v.tolist())
    assert uniq.tolist() == lu and inv.tolist() == li
    assert uniq.dtype == torch.int64 and inv.dtype == torch.int64
    ou, oi = O.id_unique(v.astype(np.uint64))
    assert np.array_equal(uniq.numpy().astype(np.uint64), ou) and np.array_equal(inv.numpy(), oi)


@pytest.mark.parametrize("self_loops", [True, False])
@pytest.mark.parametrize("n,count", [(0, 3), (1, 1), (7, 3), (257, 5), (1000, 2)])
def test_sage_block_vs_loop_and_oracle(O, n, count, self_loops):
    rng = np.random.default_rng(n * 10 + count)
    pool = np.concatenate([rng.integers(-2 ** 63, 2 ** 63 - 1, max(n, 2), dtype=np.int64), [-1, 0]])
    n_id = rng.choice(pool, n)
    nb = rng.choice(pool, n * count)
    got = FR.sage_block(torch.as_tensor(nb), torch.as_tensor(n_id), count, self_loops)
    want = loop_block(nb.tolist(), n_id.tolist(), count, self_loops)
    for g, w in zip(got, want):
        assert g.tolist() == w
    # ... and the oracle composition the existing block tests write out
    ou, oi = O.id_unique(np.concatenate([nb, n_id]).astype(np.uint64))
    assert np.array_equal(got[0].numpy().astype(np.uint64), ou)
    assert np.array_equal(got[1].numpy(), oi[len(nb):])
    assert np.array_equal(got[3].numpy(), oi if self_loops else oi[:len(nb)])


@pytest.mark.parametrize("self_loops", [True, False])
def test_full_block_vs_loop(self_loops):
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 6, 300)
    lens[::7] = 0
    idx = np.stack([np.cumsum(lens) - lens, np.cumsum(lens)], 1).astype(np.int32)
    n_id = rng.integers(-1, 80, 300)
    nb = rng.integers(-1, 120, int(lens.sum()))
    src = FR.nb_src_of_idx(torch.as_tensor(idx))
    assert src.tolist() == np.repeat(np.arange(300), lens).tolist()
    got = FR.full_block(torch.as_tensor(nb), src, torch.as_tensor(n_id), self_loops)
    uniq, inv = loop_unique(nb.tolist() + n_id.tolist())
    assert got[0].tolist() == uniq and got[1].tolist() == inv[len(nb):]
    if self_loops:
        assert got[2].tolist() == src.tolist() + list(range(300)) and got[3].tolist() == inv
    else:
        assert got[2].tolist() == src.tolist() and got[3].tolist() == inv[:len(nb)]


@pytest.mark.parametrize("self_loops", [True, False])
@pytest.mark.parametrize("M,count", [(1, 3), (5, 1), (37, 4)])
def test_batched_form_vs_per_minibatch_loop(M, count, self_loops):
    rng = np.random.default_rng(M)
    n_len = rng.integers(0, 40, M)
    n_len[0] = 9
    if M > 2:
        n_len[2] = 0                                           # an empty minibatch in the middle
    pool = np.concatenate([rng.integers(-50, 50, 30), [-1, 0]])
    n_ids = [rng.choice(pool, k) for k in n_len]
    nbs = [rng.choice(pool, k * count) for k in n_len]
    if M > 1:
        n_ids[1], nbs[1], n_len[1] = n_ids[0].copy(), nbs[0].copy(), n_len[0]    # two equal minibatches
    cat = lambda xs: torch.as_tensor(np.concatenate(xs).astype(np.int64))
    new_n_id, new_len, res, src, dst = FR.sage_block_batched(cat(nbs), cat(n_ids), torch.as_tensor(n_len), count,
                                                             self_loops)
    per = [FR.sage_block(torch.as_tensor(nbs[b]), torch.as_tensor(n_ids[b]), count, self_loops) for b in range(M)]
    assert new_len.tolist() == [p[0].numel() for p in per]
    for x, arr in enumerate((new_n_id, res, src, dst)):
        assert arr.tolist() == torch.cat([p[x] for p in per]).tolist(), FR.NAMES[x]
    # the padded form the GPU test reads back
    cap = int(max(n_len)) * (count + 1) + 3
    padded = torch.full((M, cap), -77, dtype=torch.int64)
    for b, p in enumerate(per):
        padded[b, :p[0].numel()] = p[0]
    assert torch.equal(FR.ragged(padded, new_len), new_n_id)


# ---- the comparison helper rejects every planted fault ---------------------------------------
CHUNK, LDS_CHUNKS = 1024, 8192


def small_flow(self_loops=True):
    """two hops, 300 roots x [5, 4] over a pool of 900 ids"""
    g = torch.Generator().manual_seed(3)
    n_id = torch.randint(-1, 900, (300,), generator=g)
    want = []
    for count in (5, 4):
        nb = torch.randint(-1, 900, (n_id.numel() * count,), generator=g)
        want.append(FR.sage_block(nb, n_id, count, self_loops))
        n_id = want[-1][0]
    return want


def clone(want):
    return [tuple(t.clone() for t in blk) for blk in want]


def counts_of(want):
    return [want[0][1].numel()] + [w[0].numel() for w in want]


def test_helper_accepts_the_reference_itself():
    for loops in (True, False):
        want = small_flow(loops)
        FR.compare_blocks(clone(want), counts_of(want), want)
        padded = [tuple(torch.cat([t, torch.full((11,), -5, dtype=torch.int64)]) for t in blk) for blk in want]
        got, cnt = FR.valid_prefix(padded, torch.as_tensor(counts_of(want), dtype=torch.int32), [5, 4], loops)
        FR.compare_blocks(got, cnt, want)


@pytest.mark.parametrize("hop", [0, 1])
def test_helper_rejects_swapped_new_n_id(hop):
    want = small_flow()
    got = clone(want)
    a = got[hop][0]
    a[[3, 4]] = a[[4, 3]]
    assert a[3] != a[4]
    with pytest.raises(AssertionError, match="hop %d new_n_id" % hop):
        FR.compare_blocks(got, counts_of(want), want)


@pytest.mark.parametrize("hop", [0, 1])
def test_helper_rejects_res_n_id_from_the_head(hop):
    for loops in (True, False):
        want = small_flow(loops)
        got = [list(b) for b in clone(want)]
        n = got[hop][1].numel()
        got[hop][1] = got[hop][3][:n].clone()                 # inv[:n] instead of the tail
        with pytest.raises(AssertionError, match="hop %d res_n_id" % hop):
            FR.compare_blocks(got, counts_of(want), want)


@pytest.mark.parametrize("at", [0, 777, -1])
def test_helper_rejects_one_edge_src_off_by_one(at):
    want = small_flow()
    got = clone(want)
    got[1][2][at] += 1
    with pytest.raises(AssertionError, match="hop 1 edge_src"):
        FR.compare_blocks(got, counts_of(want), want)


@pytest.mark.parametrize("layer", [0, 1, 2])
def test_helper_rejects_a_layer_count_one_short(layer):
    want = small_flow()
    cnt = counts_of(want)
    cnt[layer] -= 1
    with pytest.raises(AssertionError, match="layer sizes"):
        FR.compare_blocks(clone(want), cnt, want)
    # ... also when the arrays were cut with the short count
    padded = [tuple(torch.cat([t, t[-1:]]) for t in blk) for blk in want]
    got, c2 = FR.valid_prefix(padded, torch.as_tensor(cnt), [5, 4], True)
    with pytest.raises(AssertionError):
        FR.compare_blocks(got, c2, want)


def test_helper_rejects_ranks_shifted_from_chunk_8192_onwards():
    """A flow whose hop has more than 8192 chunks of 1024 positions (the size at which the kernels
    change from per-workgroup sums to a scan): every rank from chunk 8192 onwards one too large."""
    g = torch.Generator().manual_seed(8)
    n, count = 131_073, 63
    n_id = torch.randint(0, 200_000, (n,), generator=g)
    nb = torch.randint(0, 200_000, (n * count,), generator=g)
    want = [FR.sage_block(nb, n_id, count, True)]
    m = n * (count + 1)
    assert m > LDS_CHUNKS * CHUNK
    FR.compare_blocks(clone(want), counts_of(want), want)
    got = clone(want)
    got[0][3][LDS_CHUNKS * CHUNK:] += 1
    with pytest.raises(AssertionError, match="hop 0 edge_dst differs, first at %d" % (LDS_CHUNKS * CHUNK)):
        FR.compare_blocks(got, counts_of(want), want)
    got = clone(want)
    got[0][1][-5:] += 1                                      # the tail of V: res_n_id
    with pytest.raises(AssertionError, match="hop 0 res_n_id"):
        FR.compare_blocks(got, counts_of(want), want)


def test_batched_helper_rejects_faults():
    g = torch.Generator().manual_seed(4)
    n_len = torch.tensor([6, 0, 9, 4])
    n_id = torch.randint(-1, 30, (19,), generator=g)
    nb = torch.randint(-1, 30, (19 * 3,), generator=g)
    w = FR.sage_block_batched(nb, n_id, n_len, 3, True)
    counts = torch.stack([n_len, w[1]], 1)
    good = [(w[0], w[2], w[3], w[4])]
    FR.compare_batched(good, counts, [w])
    for x in range(4):
        bad = [tuple(t.clone() for t in good[0])]
        bad[0][x][2] += 1
        with pytest.raises(AssertionError, match=FR.NAMES[x]):
            FR.compare_batched(bad, counts, [w])
    short = counts.clone()
    short[2, 1] -= 1
    with pytest.raises(AssertionError, match="sizes of layer 1"):
        FR.compare_batched(good, short, [w])
