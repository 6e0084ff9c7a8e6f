"""Full-neighbour aggregation read straight from the graph's rows: Graph.neighbor_aggregate,
neighbor_degree and neighbor_norm (euler_gpu_neighbor_reduce / euler_gpu_neighbor_degree).

Every forward case compares three things bit for bit: the fused call, the composition of the
existing ops run on the GPU (get_full_neighbor, the self ids appended on the host, then
ops.gather_segment_reduce or ops.gcn_aggregate) and the numpy restatement
tests/neighbor_reduce_ref.py.  No table holds a NaN."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import neighbor_reduce_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
T = 3
N_NODES = 200
ROWS = 190                     # table rows: the ids 190 .. 200 lie at or past it
HUB, NOT_A_NODE = 17, 100000
ALL = [0, 1, 2]


def build_rows(O, ids, deg, rng, id_pool, extra=None):
    """(ref.Rows, oracle CSR) of a graph with the given per-(node, type) degrees"""
    seg = np.zeros(deg.size + 1, np.int64)
    seg[1:] = np.cumsum(deg.reshape(-1))
    e = int(seg[-1])
    nbr = rng.choice(id_pool, e).astype(np.uint64)
    if extra is not None:
        nbr[extra[0]] = extra[1]
    w = (rng.random(e) * 7.5 + 0.25).astype(F)
    csr = O.csr_from_raw(np.asarray(ids, np.uint64), seg, nbr, w, deg.shape[1])
    return ref.Rows(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w, deg.shape[1]), csr


def to_graph(EA, csr):
    return EA.Graph.from_csr(csr.row_id, csr.row_ptr, csr.type_end, csr.nbr, csr.prefix_w, csr.type_prefix,
                             csr.n_types)


@pytest.fixture(scope="module")
def base(EA, O):
    rng = np.random.default_rng(20251)
    ids = np.arange(1, N_NODES + 1)
    deg = rng.integers(0, 6, (N_NODES, T))
    deg[rng.random((N_NODES, T)) < 0.3] = 0
    for node, d3 in ((3, (0, 0, 0)), (4, (0, 1, 0)), (5, (3, 0, 4)), (6, (8, 0, 0)), (7, (2, 3, 4)),
                     (8, (20, 40, 5)), (HUB, (300, 450, 250))):
        deg[node - 1] = d3
    first_of_hub = int(deg[:HUB - 1].sum())
    R, csr = build_rows(O, ids, deg, rng, ids, extra=(first_of_hub + 5, NOT_A_NODE))
    assert (R.nbr >= ROWS).sum() > 20 and (R.nbr == NOT_A_NODE).sum() == 1
    return R, to_graph(EA, csr)


def table_np(rng, rows, d):
    return ((rng.random((rows, d)) * 4 - 2) * 10.0 ** rng.integers(-2, 3, (rows, d))).astype(F)


def bits(t):
    import torch
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


def norms(R, nodes, et, self_loop, rows):
    return (ref.norm_of(ref.degree(R, nodes, et, self_loop)),
            ref.norm_of(ref.degree(R, np.arange(rows), et, self_loop)))


def composed(torch, EA, G, op, table, nodes, et, kind, norm, self_loop, root, alpha, od):
    """the composition of the existing ops; the list is assembled on the host"""
    ops = EA.ops
    n, rows = len(nodes), table.shape[0]
    idx, ids, w, _t = G.get_full_neighbor(torch.as_tensor(nodes), et)
    idx, ids, w = idx.cpu().numpy(), ids.cpu().numpy(), w.cpu().numpy()
    all_ids, all_w, sp = [], [], [0]
    for i in range(n):
        all_ids.extend(ids[idx[i, 0]:idx[i, 1]])
        all_w.extend(w[idx[i, 0]:idx[i, 1]])
        if self_loop:
            all_ids.append(nodes[i])
            all_w.append(1.0)
        sp.append(len(all_ids))
    ids_t = torch.as_tensor(np.asarray(all_ids, np.int64)).cuda()
    w_t = torch.as_tensor(np.asarray(all_w, F)).cuda()
    sp_t = torch.as_tensor(np.asarray(sp, np.int64)).cuda()
    if kind == "norm" and op != "max":
        return ops.gcn_aggregate(table, ids_t, (n, rows), norm=norm, op=op, root=root, alpha=alpha, seg_ptr=sp_t,
                                 out_dtype=od)
    if kind == "norm":          # gcn_aggregate refuses max: the weights it would form, as an edge_weight
        owner = torch.repeat_interleave(torch.arange(n, device="cuda"), sp_t[1:] - sp_t[:-1])
        g = ids_t & 0xFFFFFFFF
        w_t = torch.where(g < rows, norm[0][owner] * norm[1][g.clamp(max=rows - 1)], torch.zeros((), device="cuda"))
    agg = ops.gather_segment_reduce(op, table, ids_t, n, seg_ptr=sp_t, out_dtype=od if root is None else torch.float32,
                                    edge_weight=None if kind is None else w_t)
    if root is None:
        return agg
    a, b = (F(1.0), F(1.0)) if alpha is None else (F(1.0 - alpha), F(alpha))
    return (agg * float(a) + root.float() * float(b)).to(table.dtype if od is None else od)


def check(torch, EA, R, G, op, x, nodes, et, kind=None, self_loop=False, root=None, alpha=None, out_dtype=None):
    """fused == composition == numpy, bit for bit; x / root are torch tensors on the GPU"""
    nodes = np.asarray(nodes, np.int64)
    rows = x.shape[0]
    norm_np = norms(R, nodes, et, self_loop, rows) if kind == "norm" else None
    norm = None if norm_np is None else tuple(torch.as_tensor(t).cuda() for t in norm_np)
    got = G.neighbor_aggregate(op, x, torch.as_tensor(nodes), et, weight=kind, norm=norm, self_loop=self_loop,
                               root=root, alpha=alpha, out_dtype=out_dtype)
    od = got.dtype
    assert od == (x.dtype if out_dtype is None else out_dtype) and tuple(got.shape) == (len(nodes), x.shape[1])
    a, b = (1.0, 1.0) if alpha is None else (F(1.0 - alpha), F(alpha))
    want = ref.aggregate(R, op, x.float().cpu().numpy(), nodes, et, kind, norm_np, self_loop,
                         None if root is None else root.float().cpu().numpy(), a, b)
    want = torch.from_numpy(want).to(od)
    assert np.array_equal(bits(got), bits(want)), "fused != numpy"
    comp = composed(torch, EA, G, op, x, nodes, et, kind, norm, self_loop, root, alpha, out_dtype)
    assert comp.dtype == od and np.array_equal(bits(got), bits(comp)), "fused != composition"
    return got


def some_nodes():
    return list(range(1, N_NODES + 1))


@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("kind", [None, "edge", "norm"])
@pytest.mark.parametrize("op", ["add", "max", "mean"])
def test_ops_kinds_self_loop(torch_cuda, EA, base, op, kind, self_loop):
    torch = torch_cuda
    R, G = base
    x = torch.as_tensor(table_np(np.random.default_rng(1), ROWS, 32)).cuda()
    check(torch, EA, R, G, op, x, some_nodes(), ALL, kind, self_loop)


@pytest.mark.parametrize("kind", [None, "edge", "norm"])
@pytest.mark.parametrize("alpha", [0.1, None])
def test_root_epilogue(torch_cuda, EA, base, kind, alpha):
    torch = torch_cuda
    R, G = base
    rng = np.random.default_rng(2)
    for d in (32, 6):
        x = torch.as_tensor(table_np(rng, ROWS, d)).cuda()
        root = torch.as_tensor(table_np(rng, N_NODES, d)).cuda()
        for op in ("add", "mean"):
            check(torch, EA, R, G, op, x, some_nodes(), ALL, kind, True, root=root, alpha=alpha)


@pytest.mark.parametrize("et", [[0], [2, 0], [1, 1], [0, 7], [0, 1, 2]], ids=str)
def test_type_lists(torch_cuda, EA, base, et):
    torch = torch_cuda
    R, G = base
    x = torch.as_tensor(table_np(np.random.default_rng(3), ROWS, 8)).cuda()
    for kind in (None, "edge", "norm"):
        check(torch, EA, R, G, "add", x, some_nodes(), et, kind, kind == "norm")


def test_duplicate_and_unknown_nodes(torch_cuda, EA, base):
    torch = torch_cuda
    R, G = base
    x = torch.as_tensor(table_np(np.random.default_rng(4), ROWS, 16)).cuda()
    nodes = [HUB, 5, 5, 0, 999, 7, HUB, -1, 1 << 40, 200, 199, 5]
    for kind in (None, "edge", "norm"):
        for self_loop in (False, True):
            check(torch, EA, R, G, "mean", x, nodes, ALL, kind, self_loop)
    empty = G.neighbor_aggregate("add", x, torch.zeros(0, dtype=torch.int64), ALL)
    assert tuple(empty.shape) == (0, 16)


@pytest.mark.parametrize("d", [1, 3, 32, 128, 130, 512])
def test_widths_fp32(torch_cuda, EA, base, d):
    """d 32 / 128: the vector form (8 / 32 lanes a node); 1, 3, 130: the element form; 512: dv > 64"""
    torch = torch_cuda
    R, G = base
    x = torch.as_tensor(table_np(np.random.default_rng(5 + d), ROWS, d)).cuda()
    nodes = some_nodes()[:64]
    check(torch, EA, R, G, "add", x, nodes, ALL, "edge", True)
    check(torch, EA, R, G, "max", x, nodes, [1, 0], None, False)


@pytest.mark.parametrize("dt", ["float32", "bfloat16", "float16"])
def test_table_view_off_a_16_byte_boundary(torch_cuda, EA, base, dt):
    torch = torch_cuda
    R, G = base
    dt = getattr(torch, dt)
    d = 32
    flat = torch.as_tensor(table_np(np.random.default_rng(6), ROWS + 1, d)).cuda().to(dt).reshape(-1)
    x = flat[1:1 + ROWS * d].view(ROWS, d)
    assert x.is_contiguous() and x.data_ptr() % 16 != 0
    check(torch, EA, R, G, "add", x, some_nodes()[:40], ALL, "norm", True)


@pytest.mark.parametrize("out32", [False, True])
@pytest.mark.parametrize("d", [64, 20])             # the 8-column vector form and the element form
@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
def test_sixteen_bit_tables(torch_cuda, EA, base, dt, d, out32):
    torch = torch_cuda
    R, G = base
    dt = getattr(torch, dt)
    rng = np.random.default_rng(7)
    x = torch.as_tensor((rng.random((ROWS, d)) * 4 - 2).astype(F)).cuda().to(dt)
    od = torch.float32 if out32 else None
    root16 = torch.as_tensor(table_np(rng, N_NODES, d)).cuda().to(dt)
    check(torch, EA, R, G, "add", x, some_nodes(), ALL, "edge", False, out_dtype=od)
    check(torch, EA, R, G, "mean", x, some_nodes(), ALL, None, True, out_dtype=od)
    check(torch, EA, R, G, "max", x, some_nodes(), ALL, "norm", True, out_dtype=od)
    check(torch, EA, R, G, "add", x, some_nodes(), ALL, "norm", True, root=root16, alpha=0.1, out_dtype=od)
    check(torch, EA, R, G, "add", x, some_nodes(), ALL, "norm", True, root=root16.float(), out_dtype=od)


def test_past_the_grid_cap(torch_cuda, EA, base):
    """40 000 queried nodes at d = 3: 10 000 blocks of four wave-slots, the launch has 8 192 - the
    second trip of the node loop"""
    torch = torch_cuda
    R, G = base
    rng = np.random.default_rng(8)
    x = torch.as_tensor(table_np(rng, ROWS, 3)).cuda()
    nodes = rng.integers(1, 17, 40000)           # (repeats; the hub stays out: the composition's list is small)
    nodes[-1] = 16
    nodes[8192 * 4 + 1] = 8
    check(torch, EA, R, G, "add", x, nodes, ALL, "edge", True)


def test_hashed_ids(torch_cuda, EA, O):
    """ids that are not strided, all below the table's rows: the hash map finds the rows"""
    torch = torch_cuda
    rng = np.random.default_rng(9)
    ids = np.sort(rng.choice(np.arange(1, 500), 60, replace=False))
    assert len(set(np.diff(ids))) > 1
    deg = rng.integers(0, 9, (60, 2))
    R, csr = build_rows(O, ids, deg, rng, ids)
    G = to_graph(EA, csr)
    x = torch.as_tensor(table_np(rng, 500, 12)).cuda()
    nodes = list(ids) + [2, 499, 777] + [int(i) + 1 for i in ids[:5]]
    for kind in (None, "edge", "norm"):
        check(torch, EA, R, G, "add", x, nodes, [1, 0], kind, True)
    G.close()


def test_degree_and_norm(torch_cuda, EA, base):
    torch = torch_cuda
    R, G = base
    nodes = np.array(some_nodes() + [0, 999, HUB, HUB], np.int64)
    for et in ([0], [2, 0], [1, 1], [0, 7], ALL):
        idx = G.get_full_neighbor(torch.as_tensor(nodes), et)[0].cpu().numpy()
        for self_loop in (False, True):
            want = (idx[:, 1] - idx[:, 0] + (1 if self_loop else 0)).astype(np.int32)
            assert np.array_equal(want, ref.degree(R, nodes, et, self_loop))
            deg = G.neighbor_degree(nodes, et, self_loop)
            assert deg.dtype == torch.int32 and np.array_equal(deg.cpu().numpy(), want)
            nrm = G.neighbor_norm(nodes, et, self_loop)
            assert nrm.dtype == torch.float32
            assert np.array_equal(nrm.cpu().numpy().view(np.uint32), ref.norm_of(want).view(np.uint32))
    # norm=None computes the two tables from the listed degrees
    x = torch.as_tensor(table_np(np.random.default_rng(10), ROWS, 8)).cuda()
    nd, ns = norms(R, nodes, ALL, True, ROWS)
    a = G.neighbor_aggregate("add", x, nodes, ALL, weight="norm", self_loop=True)
    b = G.neighbor_aggregate("add", x, nodes, ALL, weight="norm", self_loop=True,
                             norm=(torch.as_tensor(nd).cuda(), torch.as_tensor(ns).cuda()))
    assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("kind,op", [(None, "add"), ("edge", "mean"), ("edge", "max"), ("norm", "add"),
                                     ("norm", "mean")])
def test_gradients_equal_the_compositions(torch_cuda, EA, base, kind, op):
    torch = torch_cuda
    R, G = base
    rng = np.random.default_rng(11)
    d = 8
    nodes = np.asarray(some_nodes()[:60] + [HUB, 5, 999], np.int64)
    x0 = torch.as_tensor(table_np(rng, ROWS, d)).cuda()
    r0 = torch.as_tensor(table_np(rng, len(nodes), d)).cuda()
    g_out = torch.as_tensor(table_np(rng, len(nodes), d)).cuda()
    norm_np = norms(R, nodes, ALL, True, ROWS) if kind == "norm" else None
    norm = None if norm_np is None else tuple(torch.as_tensor(t).cuda() for t in norm_np)
    grads = []
    for fused in (True, False):
        x, r = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
        if fused:
            out = G.neighbor_aggregate(op, x, nodes, ALL, weight=kind, norm=norm, self_loop=True, root=r, alpha=0.25)
        else:
            out = composed(torch, EA, G, op, x, nodes, ALL, kind, norm, True, r, 0.25, None)
        out.backward(g_out)
        grads.append((out, x.grad, r.grad))
    for a, b in zip(*grads):
        assert np.array_equal(bits(a), bits(b))
    assert float(grads[0][1].abs().sum()) > 0 and float(grads[0][2].abs().sum()) > 0
    # the packaged composition is that composition
    pk = G.neighbor_aggregate_composed(op, x0, nodes, ALL, weight=kind, norm=norm, self_loop=True, root=r0, alpha=0.25)
    assert np.array_equal(bits(pk), bits(grads[0][0]))


def test_example_runs_in_both_modes(torch_cuda):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", "full_graph_propagate.py"),
                          "--nodes", "3000", "--edges", "30000", "--dim", "16", "--hops", "2", "--composed"],
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = run.stdout.decode()
    assert run.returncode == 0, text[-3000:]
    assert "bit-identical" in text and "fused" in text and "composed" in text
