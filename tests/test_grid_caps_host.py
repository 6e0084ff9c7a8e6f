"""The cases of test_grid_caps_gpu.py against the launch grids restated in grid_caps.py, on the CPU:
every case needs more blocks than its launcher's cap (so a block makes a second trip), is small
(at most 1.25 times the cap - the 40 000 destinations at four rows a block are 1.22 times - or the
cap plus a partial block), has something to compute in the items that only a second trip writes,
and has the share / histogram mode it claims.  If a cap, a tile or a lane rule changes in
euler_amd/csrc, grid_caps.py is changed with it and this file says which cases no longer stride."""
import numpy as np
import pytest

import grid_caps as C
from conftest import ROOT


def strided(grid, what):
    assert grid.blocks > grid.cap, (what, grid)
    assert grid.blocks <= 1.25 * grid.cap or grid.blocks <= grid.cap + 4, (what, grid)
    return grid


def source(name):
    with open("%s/euler_amd/csrc/%s" % (ROOT, name)) as f:
        return f.read()


def test_the_restated_constants_are_the_sources():
    """the caps and tile constants as the sources spell them (a reminder to look, not a parser)"""
    for name, text in (("mp_segments.h", "if (blocks > 256 * 32) blocks = 256 * 32;"),
                       ("mp_softmax.h", "if (chunks > 256 * 32) chunks = 256 * 32;"),
                       ("mp_softmax.h", "int64_t share = 2048 / chunks;"),
                       ("mp_softmax.h", "constexpr int kSmxShort = 32;"),
                       ("edge_dot_kernels.hip", "if (blocks > 256 * 32) blocks = 256 * 32;"),
                       ("edge_softmax_kernels.hip", "(blocks > 256 * 32 ? 256 * 32 : blocks)"),
                       ("segment_attention_kernels.hip", "(blocks > 256 * 64 ? 256 * 64 : blocks)"),
                       ("common.h", "const int64_t cap = 256 * 16;"),
                       ("supervise_kernels.hip", "const int64_t cap = mode == kHistLds ? 512 : 4096;"),
                       ("supervise_kernels.hip", "kSvWideRows = 256, kSvNarrowRows = 64, kSvWideMaxC = 15;"),
                       ("supervise_kernels.hip", "constexpr int kSvLdsLimit = 64 * 1024;"),
                       ("segment_topk_kernels.hip", "return blocks > (1 << 20) ? (1 << 20) : blocks;"),
                       ("fp8_rows_kernels.hip", "std::min<int64_t>((n + 3) / 4, 8192 / by)")):
        assert text in source(name), (name, text)
    assert C.SV_OFF_HIST == 19776 and C.SV_LDS_T_MAX == 5719
    assert C.SV_OFF_HIST + 8 * (C.SV_LDS_T_MAX + 1) == 64 * 1024          # exactly 64 KiB of dynamic LDS


def test_the_lane_rules():
    assert C.row_lane_shape(67, 256, 4).per_block == 4 and C.row_lane_shape(67, 4, 4).per_block == 256
    assert C.row_lane_shape(67, 512, 4).per_block == 4 and not C.row_lane_vec(512, 4)       # d / 4 > 64
    assert not C.row_lane_vec(12, 4) and not C.row_lane_vec(8, 4, dh=2) and not C.row_lane_vec(16, 8, dh=4)
    assert C.row_lane_vec(512, 8, dh=128) and C.row_lane_vec(1024, 16) and not C.row_lane_vec(256, 4, aligned=False)
    assert C.smx_long_grid(5000)[1] == 16 and C.smx_long_grid(1)[1] == 16
    assert [C.att_lanes(dh) for dh in (1, 4, 20, 256, 1024)] == [1, 1, 8, 64, 64]
    assert not C.att_short_serves(65, 1) and not C.att_short_serves(1, 512) and C.att_short_serves(1, 256)


def last_trip_has_work(lens, grid):
    """among the destinations that only a second trip writes: a non-empty one, an empty one"""
    late = lens[grid.first_trip:]
    return len(late) > 0 and (late > 0).any() and (late == 0).any()


@pytest.mark.parametrize("d,size", C.HALF_PLAIN)
def test_half_plain_cases(d, size):
    g = strided(C.row_lane_shape(size, d, 8), (d, size))
    assert g.per_block == {3: 4, 512: 4, 8: 256}[d]
    lens = C.seg_lengths(size, size + 300, long_at=(5, size - 6), long_len=(37, 21))
    assert last_trip_has_work(lens, g) and size - 6 >= g.first_trip and set(lens[:1000]) == {0, 1, 2, 37}


def test_every_reduce_case_shares_those_blocks():
    """the 16-bit, fp32 weighted and fp8 reduces all run the block of (destinations, 300 table rows)"""
    sizes = {s for *_, s in C.HALF_PLAIN + C.HALF_WEIGHTED + C.F32_WEIGHTED} | {s for _, s, _ in C.FP8_REDUCE}
    assert sizes == {C.BIG8, C.BIG256}
    for size, per_block in ((C.BIG256, 4), (C.BIG8, 256)):
        lens = C.seg_lengths(size, size + 300, long_at=(5, size - 6), long_len=(37, 21))
        assert last_trip_has_work(lens, C.Grid(C.ceil_div(size, per_block), C.ROW_CAP, per_block))
        assert lens[size - 6] == 21 and size - 6 >= C.ROW_CAP * per_block and lens[-1] == 2


@pytest.mark.parametrize("d,heads,size", C.HALF_WEIGHTED)
def test_half_weighted_cases(d, heads, size):
    g = strided(C.row_lane_shape(size, d, 8, d // heads), (d, heads, size))
    assert C.row_lane_vec(d, 8, d // heads) == (d == 512) and g.per_block == 4


@pytest.mark.parametrize("d,heads,size", C.F32_WEIGHTED)
def test_f32_weighted_cases(d, heads, size):
    g = strided(C.row_lane_shape(size, d, 4, d // heads), (d, heads, size))
    assert C.row_lane_vec(d, 4, d // heads) == (d in (256, 4))
    assert g.per_block == {3: 4, 256: 4, 8: 4, 4: 256}[d]


@pytest.mark.parametrize("d,size,out", C.FP8_REDUCE)
def test_fp8_reduce_cases(d, size, out):
    for dh in (0, d):
        g = strided(C.row_lane_shape(size, d, 16, dh), (d, size))
        assert g.per_block == {3: 4, 1024: 4, 16: 256}[d]


@pytest.mark.parametrize("d,e,out16,cache_stays", C.FP8_GATHER)
def test_fp8_gather_cases(d, e, out16, cache_stays):
    g, dv = C.fp8_gather_grid(e, d, out16)
    strided(g, (d, e))
    assert g.first_trip == 1 << 20 and dv == {12: 3, 16: 4, 48: 3, 5: 5}[d]
    if cache_stays is not None:
        assert (g.first_trip % dv == 0) == cache_stays


def test_fp8_quantize_and_absmax_cases():
    n, d = C.FP8_QUANTIZE
    strided(C.grid_for(n * d), "quantize")
    for (n, d), by in zip(C.FP8_ABSMAX, (1, 3)):
        g, blocks_y = C.column_absmax_grid(n, d)
        strided(g, (n, d))
        assert blocks_y == by and g.first_trip + 3 < n - 1


@pytest.mark.parametrize("d,heads,e", C.EDGE_DOT)
def test_edge_dot_cases(d, heads, e):
    g, v, log_l = C.edge_dot_grid(e, heads, d)
    strided(g, (d, heads, e))
    assert (v, log_l) == {512: (8, 6), 24: (4, 2), 1: (1, 0)}[d]
    assert e * heads - 37 * heads >= g.first_trip          # the tail the test runs alone is a second trip


def test_relation_and_gcn_cases():
    for dtype, d, size, R in C.RELATION_VEC:
        assert C.row_lane_vec(d, C.LANE_N[dtype])
        assert strided(C.row_lane_shape(size, d, C.LANE_N[dtype]), (dtype, d)).per_block == 4
    # 20 000 destinations x 2 relations do NOT stride: the launcher sees the destinations
    assert not C.row_lane_shape(20_000, 256, 4).strides
    d, size = C.GCN_VEC
    g = strided(C.row_lane_shape(size, d, 4), "gcn")
    assert g.blocks == g.cap + 1 and C.row_lane_vec(d, 4)
    lens = C.seg_lengths(size, size, long_at=(5, size - 1), long_len=(19, 11))
    assert lens[-1] == 11 and size - 1 == g.first_trip      # the one row of the second trip: eleven updates


def test_edge_softmax_cases():
    size, heads = C.SMX_SHORT_SIZE, C.SMX_SHORT_HEADS
    g = strided(C.smx_short_grid(size, heads), "short")
    at, n = C.smx_long_segments(size)
    lens = C.seg_lengths(size, 2, at, n, high=4)
    assert last_trip_has_work(lens, C.Grid(g.blocks, g.cap, 256 // heads)) and lens.max() == 300
    assert set(lens.tolist()) >= {0, 1, 2, 3, 33, 300}
    assert ((lens > C.SMX_SHORT)[-300:]).sum() >= 4 and ((lens > C.SMX_SHORT)[:300]).sum() >= 4
    outside, heads, fsize = C.SMX_FILL
    strided(C.smx_zero_fill_grid(outside, heads, fsize), "zero fill")
    assert C.smx_zero_fill_grid(outside, heads, fsize).cap == C.ROW_CAP          # a full grid strides
    seen = set()
    for size, share in C.SMX_LONG:
        g, got = C.smx_long_grid(size)
        assert got == share, (size, got)
        seen.add((g.strides, share))
        at, n = C.smx_long_segments(size)
        lens = C.seg_lengths(size, size, at, n)
        long = np.flatnonzero(lens > C.SMX_SHORT)
        assert len(long) == 8 and (long < 300).sum() == 4 and (long >= size - 300).sum() == 4
        assert len(set(long[:3] // 256)) == 1 and len(set(long[-2:] // 256)) == 1      # several in one chunk
        if g.strides:
            strided(g, size)
            assert (long >= g.first_trip).sum() == 4 and (lens[g.first_trip:] <= C.SMX_SHORT).any()
    assert any(1 < s < 16 for _, s in seen) and (False, 1) in seen and (True, 1) in seen
    assert {C.smx_long_grid(s)[1] for s, _ in C.SMX_LONG} >= {13, 3, 1}


def test_attention_cases():
    for (d, size, count), log_g in zip(C.ATT_SHORT, (6, 0)):
        for grad in (False, True):
            g, got = C.att_short_grid(size, 1, d, d, "dot", grad)
            strided(g, (d, size, grad))
            assert got == log_g and g.per_block == 256 >> log_g and count <= 16
    for size in C.ATT_LONG:
        g, share = C.smx_long_grid(size)
        assert (share, g.strides) == ((13, False) if size == 40_000 else (1, True))
        for kind in ("dot", "additive"):       # (256 destinations a block: the short kernel's grid does not stride here)
            short, _ = C.att_short_grid(size, 1, 1, 1, kind)
            assert not short.strides and short.per_block == 256


@pytest.mark.parametrize("mode,t,c,b", C.SUPERVISE + [C.SUPERVISE_GRAPH])
def test_supervise_cases(mode, t, c, b):
    g, got = C.supervise_grid(b, c, t)
    assert got == mode and g.cap == (512 if mode == "lds" else 4096) and g.per_block == (256 if c <= 15 else 64)
    assert g.blocks == g.cap + 2 and b % g.per_block == 1        # a whole tile and one row past the cap
    x, z = C.supervise_inputs(b, c)
    late_x, late_z = x[g.first_trip:], z[g.first_trip:]
    assert len(late_x) == g.per_block + 1
    assert ((late_z != 0) & (late_x > 0)).any() and ((late_z != 0) & (late_x < 0)).any()     # tp and fn
    assert ((late_z == 0) & (late_x > 0)).any() and ((late_z == 0) & (late_x < 0)).any()     # fp and tn


def test_supervise_histogram_limit_cases():
    assert [C.supervise_mode(t) for t in (None, 2, 5000, 5719, 5720, 6000, 20_000)] == \
        ["none", "lds", "lds", "lds", "global", "global", "global"]
    assert sorted({(t, mode) for _, _, t, mode in C.SUPERVISE_LIMIT}) == [(5719, "lds"), (5720, "global"),
                                                                         (20_000, "global")]
    assert {(b, c) for b, c, _, _ in C.SUPERVISE_LIMIT} == {(257, 3), (257, 41)}


def test_topk_case():
    g = strided(C.tk_grid(C.TOPK_SIZE), "topk")
    assert g.first_trip == 1 << 28 and C.TOPK_SIZE < 1 << 31
