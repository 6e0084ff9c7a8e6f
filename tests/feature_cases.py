"""The ragged feature layout and the query mixes shared by tests/test_feature_ref_host.py and
tests/test_features_gpu.py.  Three slots per record; the lengths cross every pass boundary of the
fill loops (8 lanes per edge, 64 per node) and every value encodes (record, slot, position), so
a value read from the wrong record, slot or position differs from the expected one."""
import numpy as np

SLOTS = 3
# around one and two passes of an 8-lane group and of a 64-lane wave, and many passes
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300)
FIDS = (-1, 0, 1, 2, 3, 7)


def ragged_lengths(n, seed):
    """[n, 3] slot lengths: every value of LENGTHS occurs in each slot; records with an empty
    middle slot between two non-empty ones; records with every slot empty; short slots
    elsewhere (the tables stay small)."""
    assert n >= 2 * SLOTS * len(LENGTHS) + 20
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 10, (n, SLOTS))
    r = 0
    for s in range(SLOTS):
        for twice in range(2):                    # (two records per length: one alone in its
            for v in LENGTHS:                     # record, one between filled neighbours)
                if twice == 0:
                    lens[r] = 0
                lens[r, s] = v
                r += 1
    lens[r:r + 10, 1] = 0                         # empty middle slot
    lens[r:r + 10, 0] = rng.integers(1, 20, 10)
    lens[r:r + 10, 2] = rng.integers(1, 20, 10)
    lens[r + 10:r + 20] = 0                       # nothing at all
    lens = lens[rng.permutation(n)]
    for s in range(SLOTS):
        assert set(LENGTHS) <= set(lens[:, s].tolist())
    assert ((lens[:, 0] > 0) & (lens[:, 1] == 0) & (lens[:, 2] > 0)).any()
    assert (lens.sum(1) == 0).any()
    return lens


def _code(r, s, n):
    """(record, slot, position) in 32 bits: record < 2^17, slot < 4, position < 2^9."""
    assert r < (1 << 17) and s < 4 and n <= 512
    return (np.uint32(r) << np.uint32(11)) | (np.uint32(s) << np.uint32(9)) | np.arange(n, dtype=np.uint32)


def float_lists(lens):
    """Finite float32 values, distinct bit patterns (a small positive exponent over the code)."""
    return [[(_code(r, s, k) + np.uint32(0x20000000)).view(np.float32) for s, k in enumerate(row)]
            for r, row in enumerate(lens.tolist())]


def u64_lists(lens):
    """Every third record's values are at or above 2^63."""
    top = np.uint64(1) << np.uint64(63)
    return [[(_code(r, s, k).astype(np.uint64) << np.uint64(20)) | np.uint64(r % 1000) |
             (top if r % 3 == 0 else np.uint64(0)) for s, k in enumerate(row)]
            for r, row in enumerate(lens.tolist())]


def byte_lists(lens):
    """bytes; position 0 of a slot is 0 or 255 in turn, the rest follows the code."""
    out = []
    for r, row in enumerate(lens.tolist()):
        rec = []
        for s, k in enumerate(row):
            b = ((np.arange(k) * 7 + r * 13 + s * 101) % 256).astype(np.uint8)
            if k:
                b[0] = 0 if (r + s) % 2 else 255
            rec.append(b.tobytes())
        out.append(rec)
    return out


def node_ids(n, seed):
    """n sorted ids in [2, 2^40): irregular gaps, none adjacent to another (so id - 1 and id + 1
    are unknown)."""
    rng = np.random.default_rng(seed)
    ids = np.unique(rng.integers(1, 1 << 38, 2 * n, dtype=np.int64))
    ids = np.sort(rng.permutation(ids)[:n]) * 4 + 2
    assert len(ids) == n
    return ids.astype(np.uint64)


def node_queries(ids, seed, n=400):
    """int64 queries: every id, repeats, 0, negative ids and ids one off a real id."""
    rng = np.random.default_rng(seed)
    ids = ids.astype(np.int64)
    known = rng.choice(ids, n)
    odd = np.array([0, -1, -2 ** 63, 2 ** 63 - 1, ids[0] - 1, ids[0] + 1, ids[-1] + 1, ids[7] - 1],
                   np.int64)
    q = np.concatenate([known[:n // 2], odd, np.repeat(ids[5], 6), known[n // 2:], ids])
    return q


def grow(q, n, seed):
    """n queries drawn from q (with its first len(q) kept in place)."""
    rng = np.random.default_rng(seed)
    more = q[rng.integers(0, len(q), n - len(q))]
    return np.concatenate([q, more])
