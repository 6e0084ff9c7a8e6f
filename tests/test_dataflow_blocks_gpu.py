"""Block construction (euler_amd/csrc/dataflow_kernels.hip: euler_gpu_sage_blocks, _multi,
euler_gpu_full_blocks) at the sizes where the code changes path: chunk, word and workgroup edges,
the LDS limit of the emit kernel, the scanned path, the launch caps of the single and the
multi-minibatch flow, the automatic choice of tuning key 62, the hash-only flow of a fifth stream,
the side slot of the all-ones id, the 1.25-slot table under load, capacities at equality, n == 0
and the refusals.  Every result is compared for exact equality with the plain-torch reference of
tests/flow_ref.py (itself checked on the host by tests/test_flow_ref_host.py), fed with the
neighbours Graph.sample_neighbor / get_full_neighbor return for the REFERENCE's own layers - ops
that other files pin to the CPU oracle and that share no code with the table, flag, scan and emit
kernels.  Each case asserts from its inputs that it reaches the boundary it is named after."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import flow_ref as FR
from conftest import ROOT, make_random_graph

pytestmark = pytest.mark.gpu

# The five sizes at which dataflow_kernels.hip changes path, and the line each was read from
# (test_constants_are_the_sources checks them against the file).
CHUNK = 1024           # :50    constexpr int kFlowChunk = 1024
LDS_CHUNKS = 8192      # :363   constexpr int kFlowLdsChunks = 8192
GRID_CAP = 65536       # :1005  grid_b = f.n_blk + 1 < 65536 ? f.n_blk + 1 : 65536
MULTI_WGS = 4096       # :1120  per_mb = 4096 / n_mb > 0 ? 4096 / n_mb : 1
ROWPOS_ROOTS = 32768   # :961   rp == 1 || (rp == 2 && n <= 32768)

N_S = 200_000
# (tuning key 60, tuning key 62): the default, the hop's own row-position table always, the
# stream's row-indexed table always, op by op
PATHS = {"default": (1, 2), "rowpos": (1, 1), "rowtable": (1, 0), "opbyop": (0, None)}
SEED = 1234


def n_blk(cap_m):
    return (cap_m + CHUNK - 1) // CHUNK


def caps_of(n, fanouts):
    """(cap_n, cap_m) of every hop: the worst-case layer and the worst-case length of V"""
    out, c = [], n
    for f in fanouts:
        out.append((c, c * (f + 1)))
        c *= f + 1
    return out


def test_constants_are_the_sources():
    src = open(os.path.join(ROOT, "euler_amd", "csrc", "dataflow_kernels.hip")).read()
    assert re.search(r"constexpr int kFlowChunk = %d;" % CHUNK, src)
    assert re.search(r"constexpr int kFlowLdsChunks = %d;" % LDS_CHUNKS, src)
    assert src.count("f.n_blk + 1 < %d ? f.n_blk + 1 : %d" % (GRID_CAP, GRID_CAP)) == 2     # sage and full flows
    assert "per_mb = %d / n_mb > 0 ? %d / n_mb : 1" % (MULTI_WGS, MULTI_WGS) in src
    assert "rp == 2 && n <= %d" % ROWPOS_ROOTS in src
    assert "if (f.n_blk <= kFlowLdsChunks)" in src
    assert "constexpr size_t kMaxFlowTables = 4;" in src


@contextlib.contextmanager
def flow_path(name):
    from euler_amd import _lib
    L = _lib.lib()
    k60, k62 = PATHS[name]
    try:
        _lib.check(L.euler_gpu_set_tuning(60, k60))
        if k62 is not None:
            _lib.check(L.euler_gpu_set_tuning(62, k62))
        yield
    finally:
        L.euler_gpu_set_tuning(60, 1)
        L.euler_gpu_set_tuning(62, 2)


@pytest.fixture(scope="module")
def graph_s(EA, O):
    """S: 200 000 nodes with ids 1..N, 2.4 M weighted edges of one type, and its oracle"""
    p = EA.synth_params(20260, N_S, 2_400_000, n_types=1, weighted=True)
    po = O.SynthParams()
    for f, _ in po._fields_:
        setattr(po, f, getattr(p, f))
    return EA.Graph.synthetic(p), O.OracleGraph(O.synth_csr(po)), p


@pytest.fixture(scope="module")
def graph_h(EA, O):
    """H: 20 000 nodes with ids drawn from 10^12, four edge types"""
    rng = np.random.default_rng(771)
    ids, seg, nbr, w, nt, nw = make_random_graph(rng, 20000, 4, max_deg=40, id_space=10 ** 12)
    csr = O.csr_from_raw(ids, seg, nbr, w, 4, nt, nw)
    G = EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w, csr.type_prefix,
                          csr.n_types, csr.node_type, csr.node_weight)
    return G, O.OracleGraph(csr), ids.astype(np.int64)


def roots_of(pool, n, rng, no_row):
    """n roots from `pool`; from 8 roots on with a duplicate, id 0 and an id without a row"""
    r = rng.choice(pool, n).astype(np.int64)
    if n >= 8:
        r[3] = r[1]
        r[5] = 0
        r[6] = no_row
    return r


def ref_flow(G, roots, metapath, fanouts, default, loops, call_id, keep_nb=False):
    """The reference's flow: its own layers through Graph.sample_neighbor with the call ids the
    flow uses, every hop through flow_ref.sage_block."""
    G.set_seed(SEED)
    layer, want, nbs = roots.reshape(-1), [], []
    for h, (et, c) in enumerate(zip(metapath, fanouts)):
        nb = G.sample_neighbor(layer, et, c, default_node=default, call_id=call_id + h)[0].reshape(-1)
        want.append(FR.sage_block(nb, layer, c, loops))
        if keep_nb:
            nbs.append(nb)
        del nb
        layer = want[-1][0]
    return (want, nbs) if keep_nb else want


def oracle_flow(O, OG, roots, metapath, fanouts, default, loops, call_id):
    """the same composition on the CPU oracle: OG.sample_neighbor + O.id_unique"""
    n_id, want = np.asarray(roots, np.int64), []
    for h, (et, c) in enumerate(zip(metapath, fanouts)):
        nb, _, _ = OG.sample_neighbor(SEED, call_id + h, n_id, et, c, default)
        nb = nb.reshape(-1)
        uq, inv = O.id_unique(np.concatenate([nb, n_id]).astype(np.uint64))
        uq, inv = uq.astype(np.int64), inv.astype(np.int64)
        src = np.repeat(np.arange(len(n_id)), c)
        if loops:
            want.append((uq, inv[len(nb):], np.concatenate([src, np.arange(len(n_id))]), inv))
        else:
            want.append((uq, inv[len(nb):], src, inv[:len(nb)]))
        n_id = uq
    return want


def run_flow(G, roots, metapath, fanouts, default, loops, call_id, sync=True):
    G.set_seed(SEED)
    if sync:
        return G.sage_blocks(roots, metapath, fanouts, default_node=default, add_self_loops=loops, call_id=call_id)
    padded, counts = G.sage_blocks(roots, metapath, fanouts, default_node=default, add_self_loops=loops,
                                   call_id=call_id, sync=False)
    return FR.valid_prefix(padded, counts, fanouts, loops)


def check_paths(G, roots, metapath, fanouts, default, loops, call_id, want, paths=tuple(PATHS), sync=True, what=""):
    for path in paths:
        with flow_path(path):
            got, cnt = run_flow(G, roots, metapath, fanouts, default, loops, call_id, sync)
        FR.compare_blocks(got, cnt, want, "%s %s loops=%s" % (what, path, loops))
        del got


def free(torch):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- A1: chunk, word and workgroup edges on both small graphs, every path ---------------------
A1_SHAPES = [(1, [1]), (255, [3]), (256, [3]), (257, [3]), (511, [1]), (512, [1]), (513, [1]),
             (1, [3, 2]), (64, [3, 2]), (342, [3, 2])]


def test_a1_valid_lengths_sit_on_the_chunk_edges():
    m = [n * (f[0] + 1) for n, f in A1_SHAPES[1:7]]
    assert m == [CHUNK - 4, CHUNK, CHUNK + 4, CHUNK - 2, CHUNK, CHUNK + 2]
    # 342 roots x [3, 2]: hop 0 is 1 368 positions (two chunks), hop 1 up to 4 104 (five)
    assert [n_blk(cm) for _cn, cm in caps_of(342, [3, 2])] == [2, 5]


@pytest.mark.parametrize("default", ["max_id+1", "all_ones"])
@pytest.mark.parametrize("which", ["S", "H"])
def test_a1_small_shapes_all_paths(EA, O, torch_cuda, graph_s, graph_h, which, default):
    """Every A1 shape x self loops on / off x the four paths == the reference, and the reference ==
    the composition on the CPU oracle (OG.sample_neighbor + O.id_unique)."""
    torch = torch_cuda
    if which == "S":
        G, OG = graph_s[0], graph_s[1]
        pool, max_id, no_row, types = np.arange(1, N_S + 1), N_S, N_S + 3, [[0], [0]]
    else:
        G, OG, pool = graph_h
        max_id, no_row, types = 10 ** 13, 10 ** 13 + 5, [[0], [2]]
    dflt = max_id + 1 if default == "max_id+1" else -1
    rng = np.random.default_rng(5)
    cases = [(roots_of(pool, n, rng, no_row), types[:len(f)], f) for n, f in A1_SHAPES]
    # no root has a row: every neighbour is the default fill
    cases.append((np.array([0] + [no_row + i for i in range(63)], np.int64), types, [3, 2]))
    if which == "H":      # two listed types per hop: the hops draw a type first (the unfused flow)
        cases.append((roots_of(pool, 342, rng, no_row), [[0, 1], [2, 3]], [3, 2]))
    for ci, (roots, metapath, fanouts) in enumerate(cases):
        rt = torch.as_tensor(roots).cuda()
        call = 100 + 10 * ci
        for loops in (True, False):
            want = ref_flow(G, rt, metapath, fanouts, dflt, loops, call)
            what = "%s n=%d %s" % (which, len(roots), fanouts)
            for w, o in zip(want, oracle_flow(O, OG, roots, metapath, fanouts, dflt, loops, call)):
                for x in range(4):
                    assert np.array_equal(w[x].cpu().numpy(), o[x]), (what, FR.NAMES[x])
            check_paths(G, rt, metapath, fanouts, dflt, loops, call, want, what=what)
            with flow_path("default"):                         # ... and the padded form with device-side counts
                got, cnt = run_flow(G, rt, metapath, fanouts, dflt, loops, call, sync=False)
            FR.compare_blocks(got, cnt, want, what + " sync=False")
        if ci == len(A1_SHAPES):
            assert int((want[0][0] == dflt).sum()) == 1 and want[0][0].numel() == 65      # 64 roots + the fill
    # the flow class (default_node = max_id + 1) over the same entry
    if default == "max_id+1":
        roots, metapath, fanouts = cases[9]
        rt = torch.as_tensor(roots).cuda()
        G.set_seed(SEED, call_id=190)
        df = EA.dataflow.SageDataFlow(G, fanouts, metapath, add_self_loops=True, max_id=max_id)(rt)
        got = [(b.n_id, b.res_n_id, b.edge_index[0], b.edge_index[1]) for b in df.blocks]
        FR.compare_blocks(got, [len(roots)] + [b.size[1] for b in df.blocks],
                          ref_flow(G, rt, metapath, fanouts, dflt, True, 190), "SageDataFlow")
        assert [b.size[0] for b in df.blocks] == [len(roots)] + [b.size[1] for b in df.blocks][:-1]


def test_a1_comparison_sees_other_draws(torch_cuda, graph_s):
    """The comparison on the device can fail: a flow drawn with the next call id is another flow."""
    torch = torch_cuda
    G = graph_s[0]
    rt = torch.as_tensor(roots_of(np.arange(1, N_S + 1), 342, np.random.default_rng(2), N_S + 3)).cuda()
    want = ref_flow(G, rt, [[0], [0]], [3, 2], -1, True, 100)
    got, cnt = run_flow(G, rt, [[0], [0]], [3, 2], -1, True, 100)
    FR.compare_blocks(got, cnt, want, "same call id")
    got, cnt = run_flow(G, rt, [[0], [0]], [3, 2], -1, True, 101)
    with pytest.raises(AssertionError):
        FR.compare_blocks(got, cnt, want, "next call id")


# ---- A2: the automatic choice of tuning key 62 -------------------------------------------------
@pytest.mark.parametrize("n", [ROWPOS_ROOTS, ROWPOS_ROOTS + 1])
def test_a2_rowpos_threshold(torch_cuda, graph_s, n):
    """Key 62 at its default gives flows of at most 32 768 roots the hop's own row-position table:
    both sides of the threshold under the default, and with the table forced on and off."""
    torch = torch_cuda
    G = graph_s[0]
    assert n in (ROWPOS_ROOTS, ROWPOS_ROOTS + 1) and PATHS["default"] == (1, 2)
    rt = torch.as_tensor(roots_of(np.arange(1, N_S + 1), n, np.random.default_rng(n), N_S + 3)).cuda()
    for loops, dflt in ((True, N_S + 1), (False, -1)):
        want = ref_flow(G, rt, [[0], [0]], [2, 2], dflt, loops, 300)
        check_paths(G, rt, [[0], [0]], [2, 2], dflt, loops, 300, want, ("default", "rowtable", "rowpos"),
                    sync=loops, what="A2 n=%d" % n)


# ---- A3 - A5: the LDS limit of the emit kernel and the scanned path ---------------------------
def test_a3_emit_lds_full(torch_cuda, graph_s):
    """131 072 roots x [63]: layer 0 is not deduplicated, so m = cap_m = 8192 * 1024 exactly -
    FlowEmitIndexKernel<false> with every entry of s_pre in use."""
    torch = torch_cuda
    G = graph_s[0]
    n, fan = 131_072, [63]
    (cap_n, cap_m), = caps_of(n, fan)
    assert cap_m == LDS_CHUNKS * CHUNK and n_blk(cap_m) == LDS_CHUNKS          # the last size that is not scanned
    rt = torch.as_tensor(roots_of(np.arange(1, N_S + 1), n, np.random.default_rng(3), N_S + 3)).cuda()
    for loops, dflt in ((True, -1), (False, N_S + 1)):
        want = ref_flow(G, rt, [[0]], fan, dflt, loops, 310)
        assert want[0][1].numel() + n * fan[0] == cap_m                         # m: every chunk is live
        check_paths(G, rt, [[0]], fan, dflt, loops, 310, want, what="A3")
        del want
    free(torch)


def test_a4_scan_every_chunk_live_then_few(torch_cuda, graph_s):
    """131 073 roots x [63, 1]: hop 0 is scanned (8 193 chunks, all live) and is not the last hop, so
    the scanned emit kernel clears hop 1's table; hop 1 is scanned with fewer than 1 024 live
    chunks (one chunk per thread of the scan, most threads idle)."""
    torch = torch_cuda
    G = graph_s[0]
    n, fan = 131_073, [63, 1]
    caps = caps_of(n, fan)
    assert caps[0][1] == 8_388_672 and n_blk(caps[0][1]) == LDS_CHUNKS + 1
    assert caps[1][1] == 16_777_344 and n_blk(caps[1][1]) > LDS_CHUNKS
    rt = torch.as_tensor(roots_of(np.arange(1, N_S + 1), n, np.random.default_rng(4), N_S + 3)).cuda()
    for loops, dflt in ((True, N_S + 1), (False, -1)):
        want = ref_flow(G, rt, [[0], [0]], fan, dflt, loops, 320)
        m1 = 2 * want[0][0].numel()
        assert CHUNK < m1 <= 400_006 and n_blk(m1) < 1024
        check_paths(G, rt, [[0], [0]], fan, dflt, loops, 320, want, what="A4")
        del want
    free(torch)


@pytest.mark.parametrize("n", [30_000, 100_000])
def test_a5_scan_some_chunks_live(torch_cuda, graph_s, n):
    """[25, 10] with a scanned second hop whose valid length is a fraction of its worst case.
    30 000 random roots (8 580 000 positions at worst): layer 1 of this power-law graph has about
    56 000 distinct nodes, 11 x that is about 600 live chunks - fewer than the scan has threads, as
    in A4.  100 000 DISTINCT roots: layer 1 holds at least the 99 997 ids that stay distinct, at
    most the graph, so 1 024 < chunks < 8 192 by construction - several chunks per thread of the
    scan."""
    torch = torch_cuda
    G = graph_s[0]
    fan = [25, 10]
    caps = caps_of(n, fan)
    assert n_blk(caps[0][1]) <= LDS_CHUNKS and n_blk(caps[1][1]) > LDS_CHUNKS
    if n == 30_000:
        assert caps[1][1] == 8_580_000
        roots = roots_of(np.arange(1, N_S + 1), n, np.random.default_rng(5), N_S + 3)
    else:
        roots = np.random.default_rng(5).permutation(N_S)[:n].astype(np.int64) + 1
        roots[3], roots[5], roots[6] = roots[1], 0, N_S + 3
        assert len(np.unique(roots)) == n - 1
        assert 1024 < n_blk(11 * (n - 3)) and n_blk(11 * (N_S + 3)) < LDS_CHUNKS
    rt = torch.as_tensor(roots).cuda()
    for loops, dflt in ((True, -1), (False, N_S + 1)):
        want = ref_flow(G, rt, [[0], [0]], fan, dflt, loops, 330)
        live = n_blk(11 * want[0][0].numel())
        assert 1 < live < 1024 if n == 30_000 else 1024 < live < LDS_CHUNKS
        check_paths(G, rt, [[0], [0]], fan, dflt, loops, 330, want, sync=not loops, what="A5 n=%d" % n)
        del want
    free(torch)


# ---- A6: more chunks than the launch has workgroups --------------------------------------------
def test_a6_flag_and_insert_stride_over_a_live_chunk(EA, torch_cuda, graph_s):
    """1 048 577 roots x [63]: m = cap_m = 67 108 928 positions, 65 537 chunks for at most 65 536
    workgroups - the flag and insert kernels take a second, live, chunk (chunk 65 536)."""
    torch = torch_cuda
    from euler_amd import _lib
    G = graph_s[0]
    n, fan = 1_048_577, [63]
    (cap_n, cap_m), = caps_of(n, fan)
    assert cap_m == 67_108_928 and n_blk(cap_m) == GRID_CAP + 1 and cap_m > GRID_CAP * CHUNK
    assert n > ROWPOS_ROOTS
    fan_a = np.asarray(fan, np.int32)
    ws = int(_lib.lib().euler_gpu_sage_blocks_workspace(n, fan_a.ctypes.data_as(C.POINTER(C.c_int32)), 1))
    outs = 8 * (cap_m + cap_n + 2 * cap_m)                    # n_id, res_n_id, edge_index
    ref = 12 * 8 * cap_m                                      # the sampler's outputs, V, sort and ranks of the reference
    free(torch)
    avail = torch.cuda.mem_get_info()[0]
    if ws + outs + ref > avail:
        pytest.skip("A6 needs %.1f GB of device memory (workspace %.1f, outputs %.1f, reference %.1f), %.1f free"
                    % ((ws + outs + ref) / 1e9, ws / 1e9, outs / 1e9, ref / 1e9, avail / 1e9))
    rt = torch.as_tensor(roots_of(np.arange(1, N_S + 1), n, np.random.default_rng(6), N_S + 3)).cuda()
    want = ref_flow(G, rt, [[0]], fan, N_S + 1, True, 340)
    assert want[0][3].numel() == cap_m                        # every chunk is live
    free(torch)
    for path in ("default", "opbyop"):
        check_paths(G, rt, [[0]], fan, N_S + 1, True, 340, want, (path,), what="A6")
        free(torch)
    del want
    free(torch)


# ---- A7: the 1.25-slot table with long probe chains -------------------------------------------
def test_a7_hash_table_near_its_load_limit(EA, O, torch_cuda):
    """Graph D: 2 016 rows of 2 000 neighbours each, every neighbour an id of its own without a row.
    2 016 roots x [25]: 52 416 positions, of which about 0.955 are distinct ids without a row, in
    the 65 536 slots FlowMask gives flows with a row table (1.25 per position): load about 0.76."""
    torch = torch_cuda
    n, d = 2016, 2000
    rng = np.random.default_rng(9)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    seg = np.arange(n + 1, dtype=np.int64) * d
    nbr = (n + 1 + np.arange(n * d)).astype(np.uint64)
    w = (rng.random(n * d) * 7.5 + 0.5).astype(np.float32)
    csr = O.csr_from_raw(ids, seg, nbr, w, 1)
    G = EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w, csr.type_prefix, 1)
    rt = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
    m = n * 26
    slots = 64
    while slots < 2 * ((m * 5 + 7) // 8):                     # FlowMask -> FlowMaskOf
        slots *= 2
    assert m == 52_416 and slots == 65_536 and slots >= 1.25 * m - 1
    for fan in ([25], [25, 2]):
        for loops, dflt in ((True, -1), (False, n * d + n + 1)):
            metapath = [[0]] * len(fan)
            want, nbs = ref_flow(G, rt, metapath, fan, dflt, loops, 350, keep_nb=True)
            v0 = torch.cat([nbs[0], rt])
            load = torch.unique(v0[(v0 > n) | (v0 < 1)]).numel() / slots
            assert 0.7 <= load <= 0.8, load
            if len(fan) == 2:                                  # hop 2: the layer's ids without a row draw the default
                assert int((nbs[1] == dflt).sum()) >= 2 * 0.85 * m
            check_paths(G, rt, metapath, fan, dflt, loops, 350, want, ("default", "rowtable", "opbyop"),
                        what="A7 %s" % fan)


# ---- A8: a fifth stream has no row-indexed table -----------------------------------------------
def test_a8_fifth_stream_takes_the_hash_only_flow(EA, torch_cuda, graph_s):
    """Flows on five streams of one fresh graph.  At most kMaxFlowTables = 4 streams of a graph get
    a row-indexed table (FlowDenseTable), so the fifth stream's flows go through
    FlowInsertKernel<true> as single flows - a path that cannot be observed from outside: it
    follows from that constant (test_constants_are_the_sources).  The same holds for full_blocks
    on that stream."""
    torch = torch_cuda
    G = EA.Graph.synthetic(graph_s[2])                         # no block call has touched this graph
    rng = np.random.default_rng(8)
    streams = [torch.cuda.Stream() for _ in range(5)]
    for (n, fan), dflt in (((342, [3, 2]), -1), ((30_000, [5, 4]), N_S + 1)):
        rt = torch.as_tensor(roots_of(np.arange(1, N_S + 1), n, rng, N_S + 3)).cuda()
        for loops in (True, False):
            want = ref_flow(G, rt, [[0], [0]], fan, dflt, loops, 360)
            torch.cuda.synchronize()
            res = []
            for s in streams:
                with torch.cuda.stream(s):
                    res.append(run_flow(G, rt, [[0], [0]], fan, dflt, loops, 360))
            torch.cuda.synchronize()
            for si, (got, cnt) in enumerate(res):
                FR.compare_blocks(got, cnt, want, "A8 stream %d n=%d" % (si, n))
            FR.compare_blocks(res[4][0], res[4][1], [b[:4] for b in res[0][0]], "A8 fifth stream against the first")
    rt = torch.as_tensor(roots_of(np.arange(1, N_S + 1), 2000, rng, N_S + 3)).cuda()
    want = ref_full(G, rt, [[0], [0]], True, True)
    torch.cuda.synchronize()
    with torch.cuda.stream(streams[4]):
        blocks, cnt = G.full_blocks(rt, [[0], [0]], [want[0][4].numel() + 100, want[1][4].numel() + 100], True, True)
    torch.cuda.synchronize()
    assert blocks is not None
    FR.compare_blocks(blocks, cnt[:3], want, "A8 full_blocks on the fifth stream")


# ---- A9 / A10: empty inputs and refusals --------------------------------------------------------
def test_a9_no_roots(torch_cuda, graph_s):
    torch = torch_cuda
    G = graph_s[0]
    none = torch.empty(0, dtype=torch.int64, device="cuda")
    for loops in (True, False):
        blocks, cnt = G.sage_blocks(none, [[0], [0]], [3, 2], default_node=-1, add_self_loops=loops, call_id=1)
        assert list(cnt) == [0, 0, 0] and len(blocks) == 2
        assert all(t.numel() == 0 for blk in blocks for t in blk)
        out = G.sage_blocks_multi(none.reshape(3, 0), [[0], [0]], [3, 2], default_node=-1, add_self_loops=loops,
                                  call_id=1)
        assert len(out) == 3
        for blocks, cnt in out:
            assert list(cnt) == [0, 0, 0] and all(t.numel() == 0 for blk in blocks for t in blk)
        blocks, cnt = G.full_blocks(none, [[0], [0]], [10, 10], loops, True)
        assert list(cnt) == [0] * 6 and all(t.numel() == 0 for blk in blocks for t in blk)


def test_a10_refusals_leave_the_counts_alone(torch_cuda, graph_s):
    """The argument checks of the C entries: a worst case above 2^29, nine layers, a fanout of 0,
    65 536 minibatches - each answers EINVAL before anything is launched (every buffer here is a
    real, small one; none of these calls may write to it)."""
    torch = torch_cuda
    from euler_amd import _lib
    L = _lib.lib()
    G = graph_s[0]
    i32p = C.POINTER(C.c_int32)
    buf = lambda: torch.zeros(64, dtype=torch.int64, device="cuda")
    roots = torch.arange(1, 2 * 65536 + 1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(multi, n, fanouts, n_mb=1):
        layers = len(fanouts)
        fan = np.asarray(fanouts, np.int32)
        et = np.zeros(layers, np.int32)
        outs = [[buf() for _ in range(layers)] for _ in range(4)]
        arrs = [(C.c_void_p * layers)(*[t.data_ptr() for t in ts]) for ts in outs]
        counts = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        args = (C.c_void_p(roots.data_ptr()), n, et.ctypes.data_as(i32p), 1, fan.ctypes.data_as(i32p), layers, -1, 1,
                C.c_void_p(ws.data_ptr())) + tuple(arrs) + (C.c_void_p(counts.data_ptr()),)
        if multi:
            rc = L.euler_gpu_sage_blocks_multi(G._h, st, SEED, 0, layers, n_mb, *args)
        else:
            rc = L.euler_gpu_sage_blocks(G._h, st, SEED, 0, *args)
        torch.cuda.synchronize()
        assert rc == _lib.EINVAL, (rc, n, fanouts, n_mb)
        assert bool((counts == 0x5A5A5A5A).all())
        assert all(not bool(t.any()) for ts in outs for t in ts)

    assert 33 * 8 ** 8 > 2 ** 29 >= 32 * 8 ** 8
    for multi in (False, True):
        call(multi, 33, [7] * 8, n_mb=2)                       # worst-case layer > 2^29
        call(multi, 2, [1] * 9, n_mb=2)                        # layers > 8
        call(multi, 2, [3, 0], n_mb=2)                         # a fanout of 0
    call(True, 2, [1], n_mb=65536)                             # n_mb > 65535


# ---- multi-minibatch flows ---------------------------------------------------------------------
def ref_multi(G, roots, types, fanouts, default, loops, call_id):
    """The batched reference: minibatch b's layer h through Graph.sample_neighbor with call id
    call_id + b * layers + h, all minibatches of a hop through ONE flow_ref.sage_block_batched."""
    G.set_seed(SEED)
    M, n = roots.shape
    layers = len(fanouts)
    layer, lens = roots.reshape(-1), torch.full((M,), n, dtype=torch.int64, device=roots.device)
    want, nbs = [], []
    for h, c in enumerate(fanouts):
        parts = layer.split(lens.tolist())
        nb = torch.cat([G.sample_neighbor(parts[b], [types[h]], c, default_node=default,
                                          call_id=call_id + b * layers + h)[0].reshape(-1) for b in range(M)])
        want.append(FR.sage_block_batched(nb, layer, lens, c, loops))
        nbs.append(nb)
        layer, lens = want[-1][0], want[-1][1]
    return want, nbs


def run_multi(G, roots, types, fanouts, default, loops, call_id):
    G.set_seed(SEED)
    padded, counts = G.sage_blocks_multi(roots, [[t] for t in types], fanouts, default_node=default,
                                         add_self_loops=loops, call_id=call_id, sync=False)
    cnt = counts.to(torch.int64)
    got = []
    for h, (n_id, res, src, dst) in enumerate(padded):
        e = cnt[:, h] * (fanouts[h] + (1 if loops else 0))
        got.append((FR.ragged(n_id, cnt[:, h + 1]), FR.ragged(res, cnt[:, h]), FR.ragged(src, e), FR.ragged(dst, e)))
    return got, cnt


def check_multi(G, roots, types, fanouts, default, loops, call_id, want, what):
    for path in ("default", "opbyop"):                        # key 60 = 1 and 0
        with flow_path(path):
            got, cnt = run_multi(G, roots, types, fanouts, default, loops, call_id)
        FR.compare_batched(got, cnt, want, "%s %s" % (what, path))
        del got


def multi_roots(torch, M, n, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    r = torch.randint(1, N_S + 1, (M, n), generator=gen, device="cuda", dtype=torch.int64)
    if n >= 8:
        r[:, 3] = r[:, 1]
        r[:, 5] = 0
        r[:, 6] = N_S + 3
    return r


def test_m1_fewer_workgroups_than_chunks(torch_cuda, graph_s):
    """130 minibatches of 1 100 roots x [5, 4]: 31 workgroups per minibatch for the 33 + 1 chunks
    the flag kernel walks in hop 2 (how many of them are live depends on the draws: the layer
    would need 6 349 of its at most 6 600 ids distinct for a 32nd live chunk - M2 is the case where
    every kernel strides over live positions); two minibatches with the same roots draw with their
    own call ids."""
    torch = torch_cuda
    G = graph_s[0]
    M, n, fan = 130, 1100, [5, 4]
    per_mb = max(MULTI_WGS // M, 1)
    assert per_mb == 31 and n_blk(caps_of(n, fan)[1][1]) + 1 == 34 > per_mb
    r = multi_roots(torch, M, n, 1)
    r[1] = r[0]
    for loops, dflt in ((True, -1), (False, N_S + 1)):
        want, nbs = ref_multi(G, r, [0, 0], fan, dflt, loops, 400)
        assert not torch.equal(nbs[0][:n * 5], nbs[0][n * 5:2 * n * 5])            # same roots, other draws
        assert int(want[0][1].min()) * 5 > 4 * CHUNK                                 # several live chunks each
        check_multi(G, r, [0, 0], fan, dflt, loops, 400, want, "M1")
    # the synchronous form: per-minibatch slices of the same result
    with flow_path("default"):
        G.set_seed(SEED)
        out = G.sage_blocks_multi(r, [[0], [0]], fan, default_node=N_S + 1, add_self_loops=False, call_id=400)
    for b in (0, 1, M - 1):
        wb = ref_flow(G, r[b], [[0], [0]], fan, N_S + 1, False, 400 + 2 * b)
        FR.compare_blocks(out[b][0], out[b][1], wb, "M1 sync minibatch %d" % b)


def test_m2_one_workgroup_per_minibatch(torch_cuda, graph_s):
    """4 100 minibatches of 300 roots x [5, 4]: per_mb is at its floor, 1 - hop 2's nine chunks on
    one workgroup.  Every minibatch's hop 2 is longer than 2 048 positions (layer 1 has 800 to 950
    ids on this graph): the flag and insert kernels (1 workgroup x 1 024) and the fused sampler +
    insert (8 x 256) take further trips over live positions in every minibatch, the emit kernel
    (4 x 1 024) in most."""
    torch = torch_cuda
    G = graph_s[0]
    M, n, fan = 4100, 300, [5, 4]
    assert MULTI_WGS // M == 0 and max(MULTI_WGS // M, 1) == 1 and n_blk(caps_of(n, fan)[1][1]) == 9
    r = multi_roots(torch, M, n, 2)
    want, _ = ref_multi(G, r, [0, 0], fan, -1, True, 410)
    m2 = want[0][1] * 5
    assert int(m2.min()) > 2 * CHUNK and int(m2.median()) > 4 * CHUNK
    check_multi(G, r, [0, 0], fan, -1, True, 410, want, "M2")
    free(torch)


def test_m3_scanned_path_in_the_second_minibatch(torch_cuda, graph_s):
    """2 minibatches of 131 073 roots x [63]: 8 193 chunks each - FlowScanKernel and the scanned
    emit kernel with blockIdx.y = 1."""
    torch = torch_cuda
    G = graph_s[0]
    M, n, fan = 2, 131_073, [63]
    assert n_blk(caps_of(n, fan)[0][1]) == LDS_CHUNKS + 1
    r = multi_roots(torch, M, n, 3)
    for loops, dflt in ((True, N_S + 1), (False, -1)):
        want, _ = ref_multi(G, r, [0], fan, dflt, loops, 420)
        check_multi(G, r, [0], fan, dflt, loops, 420, want, "M3")
        del want
    free(torch)


def test_m4_largest_grid_y(torch_cuda, graph_s):
    """65 535 minibatches of 2 roots x [1]: the largest second grid dimension the entry accepts."""
    torch = torch_cuda
    G = graph_s[0]
    M, n, fan = 65535, 2, [1]
    r = multi_roots(torch, M, n, 4)
    r[7] = r[8]
    r[9, 1] = r[9, 0]
    r[10] = 0
    r[11, 0] = N_S + 3
    want, _ = ref_multi(G, r, [0], fan, -1, True, 430)
    check_multi(G, r, [0], fan, -1, True, 430, want, "M4")
    free(torch)


# ---- full-neighbour flows ------------------------------------------------------------------------
def ref_full(G, roots, metapath, loops, with_types):
    """The reference's flow: get_full_neighbor of its own layers, every hop through
    flow_ref.full_block; the fifth entry of a block is the edge types (e_id)."""
    layer, want = roots.reshape(-1), []
    for et in metapath:
        idx, ids, _w, t = G.get_full_neighbor(layer, et)
        want.append(FR.full_block(ids, FR.nb_src_of_idx(idx), layer, loops) + (t if with_types else None,))
        layer = want[-1][0]
    return want


def check_full(G, roots, metapath, caps, want, loops, with_types, what):
    L = len(metapath)
    blocks, cnt = G.full_blocks(roots, metapath, caps, loops, with_types)
    assert blocks is not None and cnt[2 * L + 1] == 0, (what, cnt)
    n_edges = [w[3].numel() - (w[1].numel() if loops else 0) for w in want]
    assert list(cnt[L + 1:2 * L + 1]) == n_edges, (what, cnt, n_edges)
    FR.compare_blocks(blocks, cnt[:L + 1], want, what)
    for blk, w in zip(blocks, want):
        assert (blk[4] is None) == (not with_types)
        if with_types:
            assert blk[4].numel() == w[4].numel()


@pytest.mark.parametrize("roots", ["2000", "all"])
def test_f1_full_blocks_scanned(torch_cuda, graph_s, roots):
    """A caller-chosen capacity of 9 000 000 edges puts the full-neighbour flow on the scanned path:
    with a few live chunks (2 000 roots) and with thousands (every id a root)."""
    torch = torch_cuda
    G = graph_s[0]
    cap = 9_000_000
    if roots == "2000":
        rt = torch.as_tensor(roots_of(np.arange(1, N_S + 1), 2000, np.random.default_rng(12), N_S + 3)).cuda()
    else:
        rt = torch.cat([torch.arange(1, N_S + 1, device="cuda"), torch.tensor([0, N_S + 3, 17], device="cuda")])
    assert n_blk(cap + rt.numel()) > LDS_CHUNKS
    for loops in (True, False):
        for with_types in (True, False):
            want = ref_full(G, rt, [[0]], loops, with_types)
            m = want[0][1].numel() + want[0][3].numel() - (want[0][1].numel() if loops else 0)
            assert n_blk(m) < 1024 if roots == "2000" else 1024 < n_blk(m) < LDS_CHUNKS
            check_full(G, rt, [[0]], [cap], want, loops, with_types, "F1 %s" % roots)
            del want
    free(torch)


def test_f2_capacity_at_equality_and_overflow_in_hop_two(EA, O, torch_cuda, graph_h):
    """Two hops over all four edge types of H: capacities equal to the true edge counts give the
    reference's blocks, one edge less in hop 2 sets the overflow word to 2, in hop 1 to 1."""
    torch = torch_cuda
    G, OG, ids = graph_h
    rng = np.random.default_rng(13)
    roots = roots_of(ids, 300, rng, 10 ** 13 + 5)
    rt = torch.as_tensor(roots).cuda()
    metapath = [[0, 1, 2, 3], [0, 1, 2, 3]]
    # get_full_neighbor against the CPU oracle on the reference's own layers
    layer = roots
    for w in ref_full(G, rt, metapath, False, True):
        idx, nb, _w, t = OG.get_full_neighbor(layer.astype(np.uint64), metapath[0])
        uq, inv = O.id_unique(np.concatenate([nb.astype(np.int64), layer]).astype(np.uint64))
        assert np.array_equal(w[0].cpu().numpy().astype(np.uint64), uq)
        assert np.array_equal(w[3].cpu().numpy(), inv[:len(nb)]) and np.array_equal(w[4].cpu().numpy(), t)
        assert np.array_equal(w[2].cpu().numpy(), np.repeat(np.arange(len(layer)), idx[:, 1] - idx[:, 0]))
        layer = uq.astype(np.int64)
    _blocks, cnt = G.full_blocks(rt, metapath, [200_000, 2_000_000], True, False)
    E0, E1 = cnt[3], cnt[4]
    assert cnt[5] == 0 and E0 > 1000 and E1 > E0
    for loops in (True, False):
        for with_types in (True, False):
            want = ref_full(G, rt, metapath, loops, with_types)
            check_full(G, rt, metapath, [200_000, 2_000_000], want, loops, with_types, "F2 roomy")
            check_full(G, rt, metapath, [E0, E1], want, loops, with_types, "F2 capacities at equality")
            blocks, cnt = G.full_blocks(rt, metapath, [E0, E1 - 1], loops, with_types)
            assert blocks is None and cnt[5] == 2 and cnt[3] == E0 and cnt[4] == 0, cnt
            blocks, cnt = G.full_blocks(rt, metapath, [E0 - 1, E1], loops, with_types)
            assert blocks is None and cnt[5] == 1 and cnt[3] == 0, cnt
    # the flow class over the same entry (its fallback and growth logic has its own test)
    df = EA.dataflow.GCNDataFlow(G, metapath, add_self_loops=True)(rt)
    got = [(b.n_id, b.res_n_id, b.edge_index[0], b.edge_index[1]) for b in df.blocks]
    FR.compare_blocks(got, [len(roots)] + [b.size[1] for b in df.blocks], ref_full(G, rt, metapath, True, False),
                      "GCNDataFlow")
    df = EA.dataflow.RelationDataFlow(G, metapath)(rt)
    got = [(b.n_id, b.res_n_id, b.edge_index[0], b.edge_index[1], b.e_id) for b in df.blocks]
    FR.compare_blocks(got, [len(roots)] + [b.size[1] for b in df.blocks], ref_full(G, rt, metapath, False, True),
                      "RelationDataFlow")
