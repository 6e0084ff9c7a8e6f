"""The grids of the op launchers in euler_amd/csrc, restated in plain Python, and the cases the
grid-cap tests run (test_grid_caps_host.py checks the tables, test_grid_caps_gpu.py runs them).

Every launcher clamps its grid and lets the kernel loop over what is left.  A Grid holds what a
launcher computes BEFORE the clamp: the blocks the call would need, the cap, and the items (rows,
tasks, lanes, tiles ...) one block covers in one trip.  blocks > cap: at least one block makes a
second trip, and the items from cap * per_block on are written by a second trip alone.

Nothing here imports the package: the numbers are read off the sources named beside them, and a
launcher that changes must be changed here by hand - the host test then says which cases no longer
pass their cap."""
import collections

import numpy as np

Grid = collections.namedtuple("Grid", "blocks cap per_block")
Grid.first_trip = property(lambda g: g.cap * g.per_block)        # items [0, first_trip) are first trips
Grid.strides = property(lambda g: g.blocks > g.cap)

ROW_CAP = 256 * 32          # RowLaneShape, SmxLongGridFor, edge_dot, edge_softmax (short)
ATT_SHORT_CAP = 256 * 64    # the short attention kernel
GRID_FOR_CAP = 256 * 16     # GridFor (common.h)
TK_CAP = 1 << 20            # TkBlocks (segment_topk_kernels.hip)
SMX_SHORT, SMX_BLOCK = 32, 256      # mp_softmax.h: kSmxShort, kSmxBlock

LANE_N = {"f32": 4, "bf16": 8, "f16": 8, "fp8": 16}      # elements of a 16-byte lane by storage type


def ceil_div(a, b):
    return -(-a // b)


# ---- mp_segments.h: RowLaneShape ----------------------------------------------------------------
def row_lane_vec(d, n, dh=0, aligned=True):
    dv = d // n
    return d % n == 0 and 1 <= dv <= 64 and 64 % dv == 0 and dh % n == 0 and aligned


def row_lane_shape(size, d, n, dh=0, aligned=True):
    """blockDim = (64, 4): four rows a block in the element form, 4 * 64 / dv in the vector form"""
    rows = 4 * (64 // (d // n)) if row_lane_vec(d, n, dh, aligned) else 4
    return Grid(ceil_div(size, rows), ROW_CAP, rows)


# ---- mp_softmax.h: SmxLongGridFor; edge_softmax_kernels.hip: Launch -----------------------------
def smx_long_grid(size):
    """-> (Grid over chunks of 256 destinations, share = gridDim.y)"""
    chunks = ceil_div(size, SMX_BLOCK)
    share = 2048 // min(chunks, ROW_CAP)
    return Grid(chunks, ROW_CAP, SMX_BLOCK), max(1, min(16, share))


def smx_short_grid(size, heads):
    """a (destination, head) a lane, 256 a block"""
    return Grid(max(1, ceil_div(size * heads, 256)), ROW_CAP, 256)


def smx_zero_fill_grid(outside, heads, size):
    """the loop over the updates that belong to no destination runs on the short kernel's grid: the
    blocks it would need against the blocks that grid has"""
    return Grid(ceil_div(outside * heads, 256), min(ROW_CAP, smx_short_grid(size, heads).blocks), 256)


# ---- mp_attention.h, segment_attention_kernels.hip: Launch --------------------------------------
def att_chunk(dh):
    return 4 if dh % 4 == 0 else 1


def att_lanes(dh):
    chunks, l = dh // att_chunk(dh), 1
    while l < 64 and l < chunks:
        l <<= 1
    return l


def att_short_serves(heads, dh_a, dot_a=True):
    if heads > 64:
        return False
    return not dot_a or (heads * att_lanes(dh_a) <= 64 and dh_a // att_chunk(dh_a) <= 64)


def att_short_grid(size, heads, d, dv, kind="dot", grad=False):
    """-> (Grid over destinations, log_g); a group of 2^log_g lanes a destination"""
    dot_a = grad or kind == "dot"
    da, dc = (dv, d) if grad else (d, dv)       # backward: the incoming gradient's rows against v's, then k's
    dha = da // heads if dot_a else 1
    la = att_lanes(dha) if dot_a else 1
    rows_c = not (grad and kind == "additive")
    chunks_c = dc // att_chunk(dc // heads) if rows_c else 0
    assert att_short_serves(heads, dha, dot_a)
    lanes, log_g = max(heads * la, min(64, chunks_c)), 0
    while (1 << log_g) < lanes:
        log_g += 1
    groups = 256 >> log_g
    return Grid(max(1, ceil_div(size, groups)), ATT_SHORT_CAP, groups), log_g


# ---- edge_dot_kernels.hip: LaunchEdgeDot ---------------------------------------------------------
def edge_dot_grid(e, heads, d, aligned=True):
    """-> (Grid over tasks = (edge, head), V, log_l): 2^log_l lanes a task, four waves a block"""
    dh = d // heads
    v = 8 if dh % 8 == 0 and aligned else 4 if dh % 4 == 0 and aligned else 1
    chunks, log_l = dh // v, 0
    while log_l < 6 and (1 << log_l) < chunks:
        log_l += 1
    per_wave = 64 >> log_l
    return Grid(ceil_div(ceil_div(e * heads, per_wave), 4), ROW_CAP, 4 * per_wave), v, log_l


# ---- common.h: GridFor ---------------------------------------------------------------------------
def grid_for(items, block=256):
    return Grid(max(1, ceil_div(items, block)), GRID_FOR_CAP, block)


# ---- fp8_rows_kernels.hip ------------------------------------------------------------------------
def fp8_gather_grid(e, d, out16=False, aligned=True):
    """-> (Grid over lanes, dv = lanes a row): 4 codes a lane to fp32, 16 to 16 bits, else 1"""
    n = 16 if out16 else 4
    dv = d // n if d % n == 0 and aligned else d
    return grid_for(e * dv), dv


def column_absmax_grid(n, d):
    """-> (Grid over rows, column blocks = gridDim.y); blockDim = (64, 4): four rows a block"""
    by = min(ceil_div(d, 64), 1024)
    return Grid(ceil_div(n, 4), 8192 // by, 4), by


# ---- supervise_kernels.hip -----------------------------------------------------------------------
SV_OFF_HIST = 64 * 65 * 4 + 256 * 8 + 256 * 4 + 4 * 4 * 4       # kSvOffHist: 19776
SV_LDS_LIMIT = 64 * 1024
SV_LDS_T_MAX = (SV_LDS_LIMIT - SV_OFF_HIST) // 8 - 1            # 5719: the last T with the histogram in LDS


def supervise_mode(t):
    """t: thresholds, or None when no histogram is asked"""
    if t is None:
        return "none"
    return "lds" if SV_OFF_HIST + 2 * (t + 1) * 4 <= SV_LDS_LIMIT else "global"


def supervise_grid(b, c, t):
    """-> (Grid over tiles of rows, histogram mode); 256 rows a tile while c <= 15, else 64"""
    rows = 256 if c <= 15 else 64
    mode = supervise_mode(t)
    return Grid(ceil_div(b, rows), 512 if mode == "lds" else 4096, rows), mode


# ---- segment_topk_kernels.hip --------------------------------------------------------------------
def tk_grid(lanes):
    return Grid(ceil_div(lanes, 256), TK_CAP, 256)


# ---- the cases ------------------------------------------------------------------------------------
BIG8, BIG256 = 2_200_000, 40_000        # destinations past 8192 blocks of 256 rows / of 4 rows

# 16-bit reduces (mp_half_kernels.hip), plain: (d, destinations); weighted: (d, heads, destinations)
HALF_PLAIN = [(3, BIG256), (512, BIG256), (8, BIG8)]
HALF_WEIGHTED = [(512, 4, BIG256), (16, 4, BIG256)]
# fp32 weighted reduces (mp_kernels.hip: LaunchWeightedReduce)
F32_WEIGHTED = [(3, 1, BIG256), (256, 4, BIG256), (8, 4, BIG256), (4, 1, BIG8)]
# fp8 rows: reduces (d, destinations, out), plain and weighted alike (heads = 1)
FP8_REDUCE = [(3, BIG256, "f32"), (1024, BIG256, "bf16"), (16, BIG8, "f32")]
# fp8 gather: (d, e, out16, the scale cache of a lane stays put across trips)
FP8_GATHER = [(12, 350_000, False, False), (16, 263_000, False, True), (48, 350_000, True, False),
              (5, 210_000, False, None)]
FP8_QUANTIZE = (350_000, 3)
FP8_ABSMAX = [(40_000, 3), (11_000, 130)]
# edge_dot: (d, heads, e)
EDGE_DOT = [(512, 1, 33_000), (24, 2, 263_000), (1, 1, 2_100_000)]
# vector forms of relation_reduce (dtype, d, destinations, relations) and gcn_aggregate (d, destinations).
# RowLaneShape sees the DESTINATIONS, not destinations * relations: 4 rows a block at dv = 64.
RELATION_VEC = [("f32", 256, 33_000, 2), ("bf16", 512, 33_000, 2)]
GCN_VEC = (256, 32_769)
# edge_softmax
SMX_SHORT_SIZE, SMX_SHORT_HEADS = 262_200, 8
SMX_FILL = (300_000, 8, SMX_SHORT_SIZE)        # updates with keys >= size, heads, size (a full grid)
SMX_LONG = [(40_000, 13), (150_000, 3), (600_000, 1), (256 * ROW_CAP + 300, 1)]      # (size, share)
SMX_LONG_HEADS = [1, 3, 8]
# attention_aggregate, heads = 1: the short kernel (d = dv, destinations, count), the long one (destinations, d = 1)
ATT_SHORT = [(256, 66_000, 2), (1, 4_200_000, 1)]
ATT_LONG = [40_000, 256 * ROW_CAP + 300]
# supervise_loss: (mode, thresholds, c, b)
SUPERVISE = [("lds", 5, 16, 512 * 64 + 65), ("lds", 5, 3, 512 * 256 + 257),
             ("none", None, 16, 4096 * 64 + 65), ("none", None, 3, 4096 * 256 + 257),
             ("global", 6000, 16, 4096 * 64 + 65)]
SUPERVISE_LIMIT = [(257, c, t, "lds" if t <= SV_LDS_T_MAX else "global")
                   for c in (3, 41) for t in (SV_LDS_T_MAX, SV_LDS_T_MAX + 1, 20_000)]
SUPERVISE_GRAPH = ("lds", 5, 4, 512 * 256 + 257)       # labels read from a graph's dense feature
# gather_segment_topk: bf16, d = 1, k = 1, count = 1
TOPK_SIZE = (1 << 28) + 1000


def seg_lengths(size, seed, long_at=(), long_len=(), low=0, high=3):
    """lengths of `size` segments: `low` .. `high` - 1 updates each, the last three 2, 0 and 1 (so the
    last trip has non-empty ones), and the long ones placed by hand"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(low, high, size).astype(np.int64)
    lens[-1], lens[-2], lens[-3] = 2, 0, 1
    for at, n in zip(long_at, long_len):
        lens[at] = n
    return lens


def supervise_inputs(b, c, seed=0):
    """-> (logits, labels) float32 [b, c]: the draw of test_supervise_gpu (0, +-88 and a tiny negative
    planted, hard labels with soft multiples of 1 / 8 among them); the LAST two rows - the last tile,
    a second trip - hold positive labels under logits of both signs (p on both sides of 0.5), then
    negative labels under the same logits"""
    rng = np.random.default_rng(1000 * c + b % 1000 + seed)
    x = (rng.standard_normal((b, c)) * 3).astype(np.float32)
    flat = x.reshape(-1)
    flat[::7], flat[3::11], flat[5::13], flat[1::17] = 0, 88, -88, -1e-7
    z = (rng.random((b, c)) < 0.4).astype(np.float32)
    z.reshape(-1)[::5] = rng.integers(0, 9, z.reshape(-1)[::5].size) / 8.0
    sign = np.where(np.arange(c) % 2 == 0, 2.5, -2.5).astype(np.float32)
    x[-1], x[-2] = sign, -sign if c > 1 else sign
    z[-1], z[-2] = 1, 0
    if c == 1:
        x[-3], z[-3] = -2.5, 1
    return x, z


def smx_long_segments(size):
    """where the long segments of an edge_softmax / attention case lie: among the first 300 and the
    last 300 destinations (both ends of the first chunk row and of the last trip), lengths past 32
    and past 256; two in ONE chunk of 256 at each end so that a share > 1 splits them"""
    at = [3, 7, 130, 299, size - 300, size - 290, size - 40, size - 4]
    n = [33, 300, 40, 257, 35, 300, 64, 33]
    return at, n
