"""Graph.from_edges on the GPU: for every case of tests/graph_from_edges_ref.py the graph built on the
device from the edge list (A) against the graph from_csr makes from the numpy restatement's layout of
the same edges (B) - the facts and every row array as bytes, then the outputs of the seeded calls,
which are what a wrong has_zero_nbr / monotone / uniform_w flag or a wrong id map would change.

The comparisons are exact (bytes): both graphs must hold the same numbers and answer with the same
kernels.  A call that the library refuses on a case is listed in EXPECTED_REFUSALS with the words of
the refusal, and both graphs must refuse it with those words; any other refusal fails the test."""
import gc
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import graph_from_edges_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, torch, dtype=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    t = torch.from_numpy(a.copy()).cuda()
    return t if dtype is None else t.to(dtype)


def _inputs(c, torch):
    return dict(src=_dev(c["src"], torch), dst=_dev(c["dst"], torch), edge_type=_dev(c["edge_type"], torch),
                weight=_dev(c["weight"], torch), n_edge_types=c["n_edge_types"], nodes=_dev(c["nodes"], torch),
                node_type=_dev(c["node_type"], torch), node_weight=_dev(c["node_weight"], torch),
                features=None if not c["features"] else [_dev(f, torch) for f in c["features"]],
                undirected=c["undirected"])


def _from_edges(EA, name, torch, **over):
    kw = _inputs(R.get_case(name), torch)
    kw.update(over)
    return EA.Graph.from_edges(**kw)


def _from_csr(EA, name):
    return EA.Graph.from_csr(**R.get_reference(name)["csr"])


@pytest.fixture(scope="module")
def pairs(EA):
    """(A, B) per case, built once"""
    import torch
    made = {}

    def get(name):
        if name not in made:
            made[name] = (_from_edges(EA, name, torch), _from_csr(EA, name))
        return made[name]
    yield get
    for a, b in made.values():
        a.close()
        b.close()


def _flat(x):
    """every tensor / array of a result, in order, as bytes"""
    import torch
    if torch.is_tensor(x):
        return [x.detach().cpu().contiguous().view(torch.uint8).numpy().reshape(-1)]
    if isinstance(x, np.ndarray):
        return [np.ascontiguousarray(x).view(np.uint8).reshape(-1)]
    if isinstance(x, (list, tuple)):
        return [b for y in x for b in _flat(y)]
    return [np.frombuffer(repr(x).encode(), np.uint8)]


def _outcome(fn):
    """the bytes of a call's results; a refusal by the library (EulerGpuError, or the ValueError a
    wrapper turns one into) is an outcome too - both graphs must then refuse with the same words.
    Any other exception is a mistake of the test's and propagates."""
    from euler_amd._lib import EulerGpuError
    try:
        return _flat(fn())
    except (EulerGpuError, ValueError) as err:
        return "%s: %s" % (type(err).__name__, err)


# (case, call) -> a piece of the library's refusal.  Everything else must produce tensors on both graphs.
NO_EDGES = "edges_from_rows: the graph has no edges"
BAD_EDGE_WEIGHTS = "edge sampler: edge weights must be finite and >= 0"
EXPECTED_REFUSALS = {
    ("empty_edges_5_nodes", "export_edges"): NO_EDGES,
    ("empty_graph", "export_edges"): NO_EDGES,
    ("empty_graph", "sample_node"): "sample_node: total node weight is 0",      # (no node to draw)
    ("negative_weight", "export_edges"): BAD_EDGE_WEIGHTS,
    ("nan_weight", "export_edges"): BAD_EDGE_WEIGHTS,
}


def _same(what, a, b, refusal=None):
    """a, b: outcomes of the same call on A and B.  refusal: the words both must refuse with, or None:
    both must have answered, with the same bytes"""
    if isinstance(a, str) or isinstance(b, str) or refusal is not None:
        shown = [x if isinstance(x, str) else "answered" for x in (a, b)]
        print("refused:", what, "|", shown[0], "|", shown[1])
        assert refusal is not None, "%s: not expected to be refused: %s | %s" % (what, shown[0], shown[1])
        assert isinstance(a, str) and isinstance(b, str) and a == b and refusal in a, (what, refusal, shown)
        return
    assert len(a) == len(b) and len(a) > 0, what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y), "%s: output %d differs" % (what, i)


def _query_ids(ref):
    ids = ref["csr"]["row_id"]
    extra = np.array([ref["max_id"] + 1 if ref["max_id"] < (1 << 64) - 1 else 12345, 0], dtype=np.uint64)
    return np.concatenate([ids, extra])


@pytest.mark.parametrize("name", R.CASES)
def test_facts_and_rows(pairs, name):
    ref = R.get_reference(name)
    A, B = pairs(name)
    csr = ref["csr"]
    assert A.num_nodes == B.num_nodes == len(csr["row_id"])
    assert A.num_edges == B.num_edges == len(csr["nbr"])
    assert A.num_edge_types == B.num_edge_types == csr["n_edge_types"]
    assert A.num_node_types == B.num_node_types
    assert A.id_range() == B.id_range() == (ref["max_id"], ref["identity"] is not None)
    assert A.num_float_features == B.num_float_features
    ids = csr["row_id"]
    ra, rb = A.export_rows(ids), B.export_rows(ids)
    for what, x, y, z in zip(("row_ptr", "type_end", "nbr", "prefix_w", "type_prefix"), ra, rb,
                             (csr["row_ptr"], csr["type_end"], csr["nbr"], csr["prefix_w"], csr["type_prefix"])):
        print(name, what, len(x))
        assert np.array_equal(_flat(x)[0], _flat(y)[0]), what
        assert np.array_equal(_flat(x)[0], _flat(np.asarray(z, x.dtype))[0]), what + " (restatement)"


@pytest.mark.parametrize("name", R.CASES)
def test_seeded_outputs(pairs, name):
    """(the graph without rows is asked for the ids 1 and 0)"""
    import torch
    ref = R.get_reference(name)
    c = R.get_case(name)
    A, B = pairs(name)
    T = c["n_edge_types"]
    et = list(range(T))
    q = _dev(_query_ids(ref), torch)
    table = torch.randn(64, 8, generator=torch.Generator().manual_seed(5)).cuda()
    calls = [
        ("sample_neighbor", lambda g: g.sample_neighbor(q, et, 4, call_id=3)),
        ("sample_neighbor one type", lambda g: g.sample_neighbor(q, [T - 1], 3, call_id=4)),
        ("sample_fanout", lambda g: g.sample_fanout(q, [et, et], [5, 3], call_id=5)),
        ("get_full_neighbor", lambda g: g.get_full_neighbor(q, et)),
        ("get_top_k_neighbor", lambda g: g.get_top_k_neighbor(q, et, 3)),
        ("random_walk", lambda g: g.random_walk(q, [et, et, et], call_id=9)),
        ("sample_node", lambda g: g.sample_node(32, -1, call_id=2)),
        ("get_node_type", lambda g: g.get_node_type(q)),
        ("sage_blocks", lambda g: g.sage_blocks(q[:-1], [et, et], [3, 2], call_id=7)),
        ("neighbor_aggregate", lambda g: g.neighbor_aggregate("add", table, q, et, weight="edge")),
    ]
    if c["features"]:
        dims = [f.shape[1] for f in c["features"]]
        calls.append(("get_dense_feature", lambda g: g.get_dense_feature(q, list(range(len(dims))), dims)))
    for g in (A, B):
        g.set_seed(11)
    for what, call in calls:
        _same("%s: %s" % (name, what), _outcome(lambda: call(A)), _outcome(lambda: call(B)),
              EXPECTED_REFUSALS.get((name, what)))
    # the edge store over the rows: row order, then entry order
    def edges(g):
        g.edges_from_rows()
        return g.export_edges()
    _same(name + ": export_edges", _outcome(lambda: edges(A)), _outcome(lambda: edges(B)),
          EXPECTED_REFUSALS.get((name, "export_edges")))


def test_alias_tables_and_draws(pairs):
    A, B = pairs("shuffled_duplicates")
    ref = R.get_reference("shuffled_duplicates")
    import torch
    q = _dev(ref["csr"]["row_id"], torch)
    for g in (A, B):
        g.build_neighbor_alias()
        g.set_seed(3)
    _same("alias draws", _outcome(lambda: A.sample_neighbor(q, [0, 1], 5, call_id=1, method="alias")),
          _outcome(lambda: B.sample_neighbor(q, [0, 1], 5, call_id=1, method="alias")))


@pytest.mark.parametrize("name", ["features_3_64", "features_4_64"])
def test_features_in_16_bits(EA, name):
    import torch
    ref = R.get_reference(name)
    A, B = _from_edges(EA, name, torch), _from_csr(EA, name)
    q = _dev(_query_ids(ref), torch)
    dims = [f.shape[1] for f in R.get_case(name)["features"]]
    for g in (A, B):
        g.set_dense_feature_dtype(torch.bfloat16)
    _same(name, _outcome(lambda: A.get_dense_feature(q, [0, 1], dims)), _outcome(lambda: B.get_dense_feature(q, [0, 1], dims)))
    _same(name + " fp32 out", _outcome(lambda: A.get_dense_feature(q, [1, 0], dims[::-1], out_dtype=torch.float32)),
          _outcome(lambda: B.get_dense_feature(q, [1, 0], dims[::-1], out_dtype=torch.float32)))
    A.close()
    B.close()


def test_node_sampler_per_type_and_set_later(EA, pairs):
    import torch
    c = R.get_case("node_types")
    A, B = pairs("node_types")
    later = _from_edges(EA, "node_types", torch, node_sampler=False)
    later.set_node_sampler(node_types=c["node_type"], node_weights=c["node_weight"])
    assert np.array_equal(A.node_weight_sums(), B.node_weight_sums())
    for g in (A, B, later):
        g.set_seed(21)
    for node_type in (0, 1, -1):
        want = _outcome(lambda: B.sample_node(64, node_type, call_id=6))
        _same("sample_node type %d" % node_type, _outcome(lambda: A.sample_node(64, node_type, call_id=6)), want)
        _same("sample_node type %d, sampler set later" % node_type,
              _outcome(lambda: later.sample_node(64, node_type, call_id=6)), want)
    q = _dev(c["nodes"], torch)
    _same("get_node_type, sampler set later", _outcome(lambda: later.get_node_type(q)), _outcome(lambda: B.get_node_type(q)))
    later.close()


def test_edge_index_and_host_lists(EA):
    """a [2, E] edge_index as src, n_edge_types found on the device"""
    import torch
    c = R.get_case("missing_types")
    kw = _inputs(c, torch)
    ei = torch.stack([kw.pop("src"), kw.pop("dst")])
    kw["n_edge_types"] = None
    A = EA.Graph.from_edges(ei, **kw)
    B = _from_csr(EA, "missing_types")
    assert A.num_edge_types == 3
    ids = R.get_reference("missing_types")["csr"]["row_id"]
    _same("edge_index", _flat(A.export_rows(ids)), _flat(B.export_rows(ids)))
    A.close()
    B.close()


@pytest.mark.parametrize("name", ["shuffled_duplicates", "undirected_nodes", "features_3_64"])
def test_inputs_unchanged(EA, name):
    import torch
    kw = _inputs(R.get_case(name), torch)
    before = {k: (v.clone() if torch.is_tensor(v) else [f.clone() for f in v] if isinstance(v, list) else v)
              for k, v in kw.items()}
    g = EA.Graph.from_edges(**kw)
    torch.cuda.synchronize()
    for k, v in kw.items():
        if torch.is_tensor(v):
            assert torch.equal(v, before[k]), k
        elif isinstance(v, list):
            assert all(torch.equal(x, y) for x, y in zip(v, before[k])), k
    g.close()


REFUSALS = [
    ("type outside [0, T)",
     dict(src=[1, 2, 3, 1], dst=[2, 3, 1, 3], edge_type=[0, 2, 1, -1], n_edge_types=2),
     r"graph_create_from_edges: 2 edges have a type outside \[0, 2\)"),
    ("src outside nodes",
     dict(src=[1, 7, 3, 9, 9], dst=[2, 3, 8, 3, 1], nodes=[1, 2, 3]),
     r"graph_create_from_edges: 3 entries of the list .* have a src that is not in nodes"),
    ("src outside nodes, reversed half",
     dict(src=[1, 2], dst=[2, 8], nodes=[1, 2, 3], undirected=True),
     r"graph_create_from_edges: 1 entries of the list .* have a src that is not in nodes"),
    ("duplicate nodes",
     dict(src=[5, 3], dst=[3, 9], nodes=[5, 3, 5, 9]),
     r"graph_create_from_edges: an id occurs more than once in nodes \(1 repeated rows\)"),
]


@pytest.mark.parametrize("what,args,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_found_on_the_device(EA, what, args, message):
    import torch
    kw = dict(args)
    for k in ("src", "dst", "nodes"):
        if k in kw:
            kw[k] = torch.tensor(kw[k], dtype=torch.int64).cuda()
    if "edge_type" in kw:
        kw["edge_type"] = torch.tensor(kw["edge_type"], dtype=torch.int32).cuda()
    # one build that succeeds first: code objects and pools are loaded before the level is read
    EA.Graph.from_edges(torch.tensor([1, 2]).cuda(), torch.tensor([2, 1]).cuda()).close()

    def level():
        gc.collect()                    # (tensors earlier tests dropped go back now, not during the call)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
    held, free = level()
    with pytest.raises(Exception) as err:
        EA.Graph.from_edges(**kw)
    text = str(err.value)
    del err
    held_after, free_after = level()
    assert re.search(message, text), text
    assert held_after == held
    # the build's blocks come from hipMalloc, which torch's counter does not see: the device's free
    # bytes must be back as well (device-wide: a block left behind shows as less)
    print(what, "free bytes before / after:", free, free_after)
    assert free_after >= free, "the refused call left %d bytes behind" % (free - free_after)


def test_features_need_nodes(EA):
    import torch
    with pytest.raises(Exception, match="features need nodes"):
        EA.Graph.from_edges(torch.tensor([1, 2]).cuda(), torch.tensor([2, 1]).cuda(),
                            features=[torch.zeros(2, 4).cuda()])


def test_other_stream_back_to_back(EA):
    """two graphs built back to back on a stream of the caller's equal one built on the default stream"""
    import torch
    name = "long_rows"
    ref = R.get_reference(name)
    ids = ref["csr"]["row_id"]
    base = _from_edges(EA, name, torch)
    kw = _inputs(R.get_case(name), torch)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        first = EA.Graph.from_edges(**kw)
        second = EA.Graph.from_edges(**kw)
    want = _flat(base.export_rows(ids))
    q = _dev(ids, torch)
    for g in (base, first, second):
        g.set_seed(4)
    draws = _outcome(lambda: base.sample_neighbor(q, [0, 1], 4, call_id=1))
    for what, g in (("first", first), ("second", second)):
        _same(what + " rows", _flat(g.export_rows(ids)), want)
        _same(what + " draws", _outcome(lambda: g.sample_neighbor(q, [0, 1], 4, call_id=1)), draws)
    for g in (base, first, second):
        g.close()


def test_example_runs():
    """examples/python/graph_from_edges.py at a small size: it asserts the block layout its aggregation
    relies on and the bit-equality of the minibatch on both graphs"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "python", "graph_from_edges.py"),
                        "--nodes", "3000", "--edges", "30000", "--batch", "64"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "bit-equal on both graphs" in r.stdout, r.stdout
