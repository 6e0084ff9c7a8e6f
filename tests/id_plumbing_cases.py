"""Case builders and host-only models for the id-plumbing family (id_unique, idx_gather /
data_gather / sparse_gather, id_split / merge_rows, dedup_split / FrontHandle, pack_rows /
expand_packed / expand_rows), shared by test_id_plumbing_host.py (which proves from the oracle
and the models alone that the cases reach the paths they name) and test_id_plumbing_gpu.py
(which runs them).  No GPU import.

The models restate what the kernels of euler_amd/csrc/mp_kernels.hip do with an id BEFORE any
race: its hash slots and the table sizes.  Which position survives a plain-store race is
arbitrary, so the front end's row count is only bounded (dedup_row_bounds); the cases are built
so that the bounds meet wherever a test wants an exact number."""
import numpy as np

M64 = (1 << 64) - 1
ALL_ONES = M64                          # the ID_UNIQUE table's empty marker
GOLDEN2 = 0x9E3779B97F4A7C15            # DedupSlot2's second-hash constant
FRONT_CHUNK = 2048                      # kFrontChunk
MAX_SHARDS = 64                         # kMaxShards
GRID_CAP_BLOCKS = 4096                  # GridFor: at most 256 * 16 workgroups of 256 threads
GRID_CAP_THREADS = GRID_CAP_BLOCKS * 256


def u64(*parts):
    """Concatenate as uint64 (numpy would promote a mix of int64 and uint64 to float64)."""
    return np.concatenate([np.asarray(p, np.uint64).reshape(-1) for p in parts]) if parts \
        else np.zeros(0, np.uint64)


def mix64(z):
    """Mix64 of euler_amd/csrc/common.h on a Python int"""
    z &= M64
    z ^= z >> 30
    z = z * 0xbf58476d1ce4e5b9 & M64
    z ^= z >> 27
    z = z * 0x94d049bb133111eb & M64
    return z ^ (z >> 31)


def mix64_np(a):
    """mix64 over a uint64 array"""
    z = np.asarray(a, np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30); z *= np.uint64(0xbf58476d1ce4e5b9)
        z ^= z >> np.uint64(27); z *= np.uint64(0x94d049bb133111eb)
        z ^= z >> np.uint64(31)
    return z


def unique_cap(n):
    """slots of the ID_UNIQUE table for n positions (plus one side slot)"""
    cap = 64
    while cap < 2 * n:
        cap *= 2
    return cap


def front_cap(n):
    """slots of each of the front end's two hash tables for n positions"""
    cap = 1024
    while cap < 4 * n:
        cap *= 2
    return cap


def slot1(id_, cap):
    return (mix64(id_) & 0xFFFFFFFF) & (cap - 1)


def slot2(id_, cap):
    return ((mix64(id_ ^ GOLDEN2) >> 20) & 0xFFFFFFFF) & (cap - 1)


def slot1_np(ids, cap):
    return (mix64_np(ids) & np.uint64(0xFFFFFFFF) & np.uint64(cap - 1)).astype(np.int64)


def slot2_np(ids, cap):
    h = mix64_np(np.asarray(ids, np.uint64) ^ np.uint64(GOLDEN2)) >> np.uint64(20)
    return (h & np.uint64(0xFFFFFFFF) & np.uint64(cap - 1)).astype(np.int64)


def _alone(keys):
    """mask: the key of this entry occurs once in keys"""
    _, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    return cnt[inv] == 1


def dedup_row_bounds(eff_ids, cap):
    """(lo, hi) for the rows the hashed front end may emit for the effective ids eff_ids with
    tables of cap slots.  lo: the distinct ids.  hi: an id alone in its first-round slot always
    merges (1 row); of the ids in shared first-round slots, one whose second-round slot is
    shared with no other such id merges too (it wins round 1 or is the only writer of its
    round-2 slot); every other id may be left with one row per position."""
    ids, mult = np.unique(np.asarray(eff_ids, np.uint64), return_counts=True)
    lo = len(ids)
    if lo == 0:
        return 0, 0
    shared = ~_alone(slot1_np(ids, cap))
    rows = np.ones(lo, np.int64)
    if shared.any():
        contested = ~_alone(slot2_np(ids[shared], cap))
        sub = rows[shared]
        sub[contested] = mult[shared][contested]
        rows[shared] = sub
    return lo, int(rows.sum())


def emulate_front_rows(eff_ids, cap, rng, stale=None):
    """Sequential emulation of DedupIdsMarkKernel, DedupIdsMark2Kernel and DedupRep: the
    positions write their slots in a random order (one of the orders the plain-store races
    allow).  stale: what a previous call left in the second table (any uint32 values).  Returns
    the number of positions that represent themselves = rows emitted."""
    ids = np.asarray(eff_ids, np.uint64)
    n = len(ids)
    s1, s2 = slot1_np(ids, cap), slot2_np(ids, cap)
    owner = np.zeros(cap, np.int64)
    owner2 = np.zeros(cap, np.int64) if stale is None else np.asarray(stale, np.int64).copy()
    for i in rng.permutation(n):
        owner[s1[i]] = i
    for i in rng.permutation(n):
        if ids[owner[s1[i]]] != ids[i]:
            owner2[s2[i]] = i
    rows = 0
    for i in range(n):
        o = owner[s1[i]]
        if ids[o] == ids[i]:
            rep = o
        else:
            o2 = owner2[s2[i]]
            rep = o2 if o2 < n and ids[o2] == ids[i] else i
        rows += rep == i
    return int(rows)


def effective_ids(ids, mask=None, group=1):
    """the ids the front end works on: positions of a masked group count as id 0"""
    eff = np.asarray(ids, np.uint64).copy()
    if mask is not None:
        eff[np.repeat(np.asarray(mask, np.uint8), max(group, 1))[:len(eff)].astype(bool)] = 0
    return eff


# ------------------------------------------------------------------------------------------
# A. id_unique
# ------------------------------------------------------------------------------------------
def distinct_ids(n, seed):
    """n distinct ids over the whole 64-bit range, never the all-ones id"""
    rng = np.random.default_rng(seed)
    out = np.unique(rng.integers(0, M64, 2 * n + 8, dtype=np.uint64))
    assert len(out) >= n
    return rng.permutation(out)[:n]


def probe_wrap_ids():
    """15 ids whose home is the LAST slot of the 64-slot table, the all-ones id twice, the 15
    again in reverse: 32 positions, so the table has 64 slots and 14 ids wrap to slot 0 .."""
    home = [i for i in range(1, 5001) if mix64(i) & 63 == 63][:15]
    return u64(home, [ALL_ONES, ALL_ONES], home[::-1])


def unique_cases():
    """{name: uint64 ids}"""
    rng = np.random.default_rng(101)
    c = {"n0": u64(), "n1": u64([42]), "n1_all_ones": u64([ALL_ONES])}
    for n in (32, 33, 255, 256, 257):
        c["distinct_%d" % n] = distinct_ids(n, 200 + n)
    c["same_257"] = np.full(257, 0x1234567, np.uint64)
    c["all_ones_257"] = np.full(257, ALL_ONES, np.uint64)
    c["probe_wrap"] = probe_wrap_ids()
    c["bit63"] = u64([5, 5 | 1 << 63, 0, 1 << 63, 5, 0, 1 << 63, 5 | 1 << 63])
    c["high_bits"] = u64([7, 7 | 1 << 32, 7 | 1 << 40, 7 | 1 << 62, 7, 0, 7 | 1 << 32, 1 << 32, 0])
    c["all_ones_first"] = u64([ALL_ONES, 3, 0, 3, ALL_ONES - 1, ALL_ONES])
    c["all_ones_last"] = u64([3, 0, ALL_ONES - 1, 3, ALL_ONES])
    c["pool3_70001"] = rng.choice(u64([9, 1 << 63, ALL_ONES]), 70001)
    c["distinct_70001"] = distinct_ids(70001, 300)
    return c


# ------------------------------------------------------------------------------------------
# B. idx_gather / data_gather / sparse_gather
# ------------------------------------------------------------------------------------------
SEG_LENS = (0, 1, 15, 16, 17, 33, 0)          # around the 16 lanes that serve a row
GATHERS = {
    "repeats": [5, 5, 2, 4, 4, 3, 1, 5],
    "reverse": [6, 5, 4, 3, 2, 1, 0],
    "only_empty": [0, 6, 0],
    "none": [],
}
GATHER_DTYPES = ("uint8", "bool", "int32", "float32", "int64", "float64")
BIG_GATHER_ROWS = 65537 + 4096                # GridFor(rows * 16, 256) caps at 65 536 rows a pass


def seg_idx(lens):
    """[n, 2] int32 (begin, end) of back-to-back segments"""
    ends = np.cumsum(np.asarray(lens, np.int64))
    return np.stack([ends - lens, ends], 1).astype(np.int32)


def gather_data(dtype, total, seed=7):
    """total elements of dtype; floats carry NaNs with payload, -0.0 and infinities"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return rng.integers(0, 2, total).astype(np.bool_)
    if dt.kind == "f":
        bits = np.dtype("u%d" % dt.itemsize)
        a = rng.standard_normal(total).astype(dt)
        b = a.view(bits)
        if dt.itemsize == 4:
            special = [0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 1]
        else:
            special = [0x7FF8000000000001, 0xFFF8000012345678, 0x7FF0000000000001,
                       0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 1]
        for k, s in enumerate(special):
            b[(1 + 5 * k) % max(total, 1)::41] = s
        return a
    info = np.iinfo(dt)
    a = rng.integers(info.min, info.max, total, dtype=dt, endpoint=True)
    a[:2] = (info.min, info.max)
    return a


def bits_of(a):
    """the array's bit pattern as unsigned integers of its item size"""
    a = np.ascontiguousarray(a)
    return a.view(np.dtype("u%d" % a.dtype.itemsize))


def big_gather_case(seed=8):
    """(idx, gather_idx): BIG_GATHER_ROWS gathered rows over 1000 segments of 0 .. 3 entries"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 4, 1000)
    return seg_idx(lens), rng.integers(0, 1000, BIG_GATHER_ROWS).astype(np.int32)


def sparse_cases():
    """{name: (gather_idx, indices [nnz, cols] int64, values, dense_shape)}"""
    rng = np.random.default_rng(9)
    row_len = [3, 0, 40, 1, 0, 17]
    rows = np.repeat(np.arange(len(row_len)), row_len)
    ind = np.stack([rows, rng.integers(0, 50, len(rows))], 1).astype(np.int64)
    gi = np.array([2, 2, 1, 5, 0, 4, 3, 2], np.int64)
    return {
        "row_of_40_int64": (gi, ind, rng.integers(-2 ** 62, 2 ** 62, len(rows)), [6, 50]),
        "float64_values": (gi, ind, gather_data("float64", len(rows)), [6, 50]),
        "nnz0": (np.array([1, 0, 1], np.int64), np.zeros((0, 2), np.int64), np.zeros(0, np.int64), [2, 50]),
    }


# ------------------------------------------------------------------------------------------
# C. id_split / merge_rows
# ------------------------------------------------------------------------------------------
SPLIT_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 513)
SPLIT_SHAPES = ((1, 1), (7, 2), (64, 64), (3, 64), (2 ** 31 - 1, 63))     # (partitions, shards)
BIG_MERGE_ROWS, BIG_MERGE_WORDS = 262145, 5     # x 5 words > GRID_CAP_THREADS: a second pass


def split_ids(n, seed=17):
    """n ids over the whole unsigned range: at and above 2^63 and the all-ones id among them"""
    rng = np.random.default_rng(seed + n)
    ids = rng.integers(0, M64, n, dtype=np.uint64, endpoint=True)
    ids[1::5] >>= np.uint64(40)                  # small ids too: every shard of (64, 64) is met
    ids[2::7] = np.uint64(ALL_ONES)
    ids[3::11] = np.uint64(1 << 63)
    if n:
        ids[-1] = np.uint64(ALL_ONES)
    return ids


def one_owner_ids(n, partitions, shards, seed=19):
    """n multiples of partitions * shards: owner 0 in every lane of every wave"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 40, n).astype(np.uint64)) * np.uint64(partitions * shards)


# ------------------------------------------------------------------------------------------
# D. dedup_split / FrontHandle
# ------------------------------------------------------------------------------------------
FRONT_SIZES = (0, 1, 2047, 2048, 2049, 4097)
ROUND2_COPIES = 40
BIG_FRONT_N = (1 << 20) + 2049                  # a second pass of the mark / place kernels, an odd tail


def pool_ids(n, pool, seed):
    """n positions drawn from `pool` distinct ids (every pool id at least once when n allows)"""
    rng = np.random.default_rng(seed)
    p = distinct_ids(pool, seed + 1)
    ids = rng.choice(p, n)
    k = min(n, pool)
    ids[:k] = p[:k]
    return rng.permutation(ids)


def round2_ids(cap=1024, count=6):
    """`count` ids with the same first-round slot and pairwise different second-round slots at
    `cap`: round 1 merges one of them, round 2 the others"""
    cand = np.arange(1, 200001, dtype=np.uint64)
    s1, s2 = slot1_np(cand, cap), slot2_np(cand, cap)
    for s in range(cap):
        cls = np.flatnonzero(s1 == s)
        _, first = np.unique(s2[cls], return_index=True)
        if len(first) >= count:
            return cand[cls[np.sort(first)[:count]]]
    raise AssertionError("no class of %d ids" % count)


def round2_case(cap=1024, seed=23):
    """ROUND2_COPIES copies of each id of round2_ids, shuffled: 240 positions"""
    ids = np.repeat(round2_ids(cap), ROUND2_COPIES)
    return np.random.default_rng(seed).permutation(ids)


def double_collision_ids(cap=1024):
    """(a, b, c): one first-round slot for all three, b and c share their second-round slot too,
    a's is another"""
    cand = np.arange(1, 200001, dtype=np.uint64)
    s1, s2 = slot1_np(cand, cap), slot2_np(cand, cap)
    for s in range(cap):
        cls = np.flatnonzero(s1 == s)
        vals, cnt = np.unique(s2[cls], return_counts=True)
        if (cnt >= 2).any() and len(vals) >= 2:
            twin = vals[cnt >= 2][0]
            b, c = cls[s2[cls] == twin][:2]
            a = cls[s2[cls] != twin][0]
            return cand[[a, b, c]]
    raise AssertionError("no double collision")


def double_collision_case(cap=1024, seed=29):
    ids = np.repeat(double_collision_ids(cap), ROUND2_COPIES)
    return np.random.default_rng(seed).permutation(ids)


def mask_cases():
    """{name: (ids, mask, root_group)}: 25 positions in groups of 10 - a mask of 3 bytes, the
    last group short"""
    ids = distinct_ids(25, 31)
    ids[ids == 0] = 1
    with_zero = ids.copy()
    with_zero[[9, 20]] = 0                                # a real id 0 beside the masked group
    rng = np.random.default_rng(37)
    return {
        "none_set": (ids, np.zeros(3, np.uint8), 10),
        "all_set": (ids, np.ones(3, np.uint8), 10),
        "middle_set": (ids, np.array([0, 1, 0], np.uint8), 10),
        "real_zero_beside_mask": (with_zero, np.array([0, 1, 0], np.uint8), 10),
        "group_of_1": (pool_ids(300, 20, 41), (rng.random(300) < 0.3).astype(np.uint8), 1),
        "nonzero_byte": (ids, np.array([0, 0, 0x80], np.uint8), 10),
    }


def dense_cases():
    """{name: (ids, table entries)}: the id-indexed table has limit + 1 entries"""
    return {
        "limit_1": (u64([0, 1, 5, ALL_ONES, 0, 5, 1, ALL_ONES, 0]), 2),
        "limit_5": (u64([4, 5, 6, 4, 6, 5, 0, 4]), 6),
    }


# ------------------------------------------------------------------------------------------
# E. pack_rows / expand_packed / expand_rows
# ------------------------------------------------------------------------------------------
def wire_rows(m, count, seed=43):
    """(ids int64 [m, count], w float32, t int32, mask uint8 [m]): negative and all-ones ids,
    types -1, weights with NaN payloads, -0.0 and infinities"""
    rng = np.random.default_rng(seed + 7 * m + count)
    ids = rng.integers(-2 ** 63, 2 ** 63 - 1, (m, count), dtype=np.int64)
    ids.reshape(-1)[::3] = -1
    ids.reshape(-1)[1::5] = -2 ** 63
    w = gather_data("float32", m * count, seed + 1).reshape(m, count)
    t = rng.integers(-1, 9, (m, count)).astype(np.int32)
    t.reshape(-1)[::4] = -1
    mask = (rng.random(m) < 0.4).astype(np.uint8)
    mask[0] = 1
    return ids, w, t, mask


def wire_pos(m, n, seed=47):
    """n positions over m rows: repeats, and - with m > 2 - rows nobody asks for"""
    rng = np.random.default_rng(seed + m + n)
    used = np.arange(m) if m <= 2 else np.flatnonzero(np.arange(m) % 3 != 1)
    pos = rng.choice(used, n).astype(np.int32)
    if n >= 2:
        pos[-1] = pos[0]
    return pos
