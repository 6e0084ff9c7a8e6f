"""Graph.from_edges without a GPU.

1. The numpy restatement of the contract (tests/graph_from_edges_ref.py) against the C restatement of
   Node::Init (oracle.csr_from_raw) on every case of the table, bit for bit: what the GPU tests
   compare the device build with is itself held to the oracle here.
2. The argument ladder of euler_gpu_graph_create_from_edges through the C ABI, in one child process
   that sees no GPU (the method of tests/test_fp8_entry_args_host.py): return code and full message
   of every rule, in ladder order.  The pointers are made-up addresses nothing dereferences - the
   ladder is host arithmetic in front of the first HIP call; a call that passes it ends in a HIP
   error (rc -3: no device), not in a kernel."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import graph_from_edges_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement vs the oracle
@pytest.mark.parametrize("name", R.CASES)
def test_restatement_equals_oracle(O, name):
    c = R.get_case(name)
    ref = R.get_reference(name)
    row_id, seg_ptr, nbr, w = ref["raw"]
    o = O.csr_from_raw(row_id, seg_ptr, nbr, w, c["n_edge_types"])
    csr = ref["csr"]
    assert np.array_equal(o.row_ptr, csr["row_ptr"])
    assert np.array_equal(o.type_end.reshape(-1), csr["type_end"])
    assert np.array_equal(np.asarray(o.nbr, np.uint64), csr["nbr"])
    assert np.array_equal(np.asarray(o.prefix_w, np.float32).view(np.uint32), csr["prefix_w"].view(np.uint32))
    assert np.array_equal(np.asarray(o.type_prefix, np.float32).reshape(-1).view(np.uint32),
                          csr["type_prefix"].view(np.uint32))


def test_cases_are_what_they_claim():
    """the properties the table's names promise, so that a case cannot quietly stop testing its edge"""
    ref = {n: R.get_reference(n) for n in R.CASES}
    deg = lambda n: np.diff(ref[n]["csr"]["row_ptr"])
    assert len(ref["empty_graph"]["csr"]["row_id"]) == 0 and len(ref["empty_edges_5_nodes"]["csr"]["row_id"]) == 5
    d = deg("isolated_rows")
    assert d[0] == 0 and d[3] == 0 and d[-1] == 0 and d[1] > 0
    assert (deg("ids_only_as_dst") == 0).sum() == 3
    te = ref["missing_types"]["csr"]["type_end"].reshape(-1, 3)
    assert te[0, 0] == 0 and te[1, 1] == te[1, 0] and te[2, 2] == te[2, 1] and te[3, 0] == 0 and te[3, 2] == te[3, 1]
    p = ref["order_sensitive_sums"]["csr"]["prefix_w"]
    rp = ref["order_sensitive_sums"]["csr"]["row_ptr"]
    assert p[rp[1] - 1] == 2.0 ** 24 and p[rp[2] - 1] == 2.0 ** 24 + 2       # (2^24 + 1) + 1 vs (1 + 1) + 2^24
    assert p[rp[3] - 1] == 2.0 ** 24 and p[rp[4] - 1] == 2.0 ** 24 + 2
    assert sorted(deg("long_rows"))[-6:] == [64, 65, 300, 1024, 1025, 70000]
    assert ref["weight_none"]["uniform_w"] and ref["long_row_unweighted"]["uniform_w"]
    assert not ref["long_rows"]["uniform_w"] and ref["long_rows"]["monotone"]
    assert not ref["negative_weight"]["monotone"] and not ref["nan_weight"]["monotone"]
    assert ref["zero_nbr"]["has_zero_nbr"] and ref["zero_id_row"]["has_zero_nbr"] and not ref["one_edge"]["has_zero_nbr"]
    assert ref["zero_id_row"]["identity"] is None and int(ref["zero_id_row"]["csr"]["row_id"][0]) == 0
    assert ref["ids_1_to_n"]["identity"] == (1, 1) and ref["ids_strided"]["identity"] == (10, 3)
    assert ref["single_row"]["identity"] == (7, 1)
    assert ref["ids_u64"]["identity"] is None and ref["nodes_descending"]["identity"] is None
    ids = ref["ids_u64"]["csr"]["row_id"]
    assert int(ids[-1]) == (1 << 64) - 1 and int(ids[0]) == 3 and ref["ids_u64"]["max_id"] == (1 << 64) - 1
    for name, keys in (("keys_power_of_two", 32), ("keys_power_of_two_plus_1", 33)):
        c = R.get_case(name)
        assert len(c["nodes"]) * c["n_edge_types"] == keys
    c = R.get_case("undirected_self_loop")
    assert ref["undirected_self_loop"]["csr"]["row_ptr"][-1] == 2 * len(c["src"])


# ------------------------------------------------------------------------------ the argument ladder
S, D, TY, W, N, NT, NW, F0, F1 = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000
BASE = dict(edges=True, out=True, n_edges=8, n_nodes=4, T=2, undirected=0, src=S, dst=D, type=TY, weight=W, nodes=N,
            node_type=NT, node_weight=NW, n_node_types=2, node_sampler=1, n_features=1, features=[F0], dims=[4])
WHO = "graph_create_from_edges: "
NULL, NEG = WHO + "null argument", WHO + "negative size"
TYPES, NTYPES = WHO + "need 1..32 edge types", WHO + "need 0..32 node types (0 = 1)"
ENDS = WHO + "null src or dst"
FEAT_NODES = WHO + "features need nodes (the rows' order is what places them)"
NODE_NODES = WHO + "node_type and node_weight need nodes (the rows' order is what places them)"
FEAT_NULL, FEAT_DIM = WHO + "null feature array", WHO + "a feature width < 1"
FEAT_SUM = WHO + "the feature widths sum to 2^31 or more"
ALIGN = WHO + "a buffer is not aligned to its type"
COUNT = WHO + "the list (E entries, 2 E when undirected) must have fewer than 2^31 entries"
NO_NODES = dict(nodes=None, node_type=None, node_weight=None, n_features=0, features=None, dims=None)
E31, E30 = 1 << 31, 1 << 30

# (changes to the base call, rc, text); rc -3: the ladder let the call through to the first HIP call
ROWS = [
    (dict(), -3, None),
    (dict(edges=False), -1, NULL),
    (dict(out=False), -1, NULL),
    (dict(n_edges=-1), -1, NEG),
    (dict(n_nodes=-1), -1, NEG),
    (dict(n_features=-1), -1, NEG),
    (dict(NO_NODES, n_nodes=-1), -3, None),              # n_nodes is not looked at without nodes
    (dict(T=0), -1, TYPES),
    (dict(T=-1), -1, TYPES),
    (dict(T=33), -1, TYPES),
    (dict(T=32), -3, None),
    (dict(n_node_types=-1), -1, NTYPES),
    (dict(n_node_types=33), -1, NTYPES),
    (dict(n_node_types=0), -3, None),
    (dict(src=None), -1, ENDS),
    (dict(dst=None), -1, ENDS),
    (dict(n_edges=0, src=None, dst=None, type=None, weight=None), -3, None),   # E = 0 is a graph
    (dict(n_nodes=0), -3, None),                                                # ... and so is N = 0
    (dict(nodes=None), -1, FEAT_NODES),
    (dict(nodes=None, n_features=0), -1, NODE_NODES),
    (dict(nodes=None, n_features=0, node_type=None), -1, NODE_NODES),
    (dict(NO_NODES), -3, None),
    (dict(features=None), -1, FEAT_NULL),
    (dict(dims=None), -1, FEAT_NULL),
    (dict(features=[None]), -1, FEAT_NULL),
    (dict(n_nodes=0, features=[None]), -3, None),        # no row, no values
    (dict(dims=[0]), -1, FEAT_DIM),
    (dict(n_features=2, features=[F0, F1], dims=[4, -1]), -1, FEAT_DIM),
    (dict(n_features=2, features=[F0, F1], dims=[E30, E30]), -1, FEAT_SUM),
    (dict(n_features=2, features=[F0, F1], dims=[E30, E30 - 1]), -3, None),
    (dict(src=S + 4), -1, ALIGN),
    (dict(dst=D + 1), -1, ALIGN),
    (dict(nodes=N + 4), -1, ALIGN),
    (dict(type=TY + 2), -1, ALIGN),
    (dict(weight=W + 1), -1, ALIGN),
    (dict(node_type=NT + 2), -1, ALIGN),
    (dict(node_weight=NW + 3), -1, ALIGN),
    (dict(features=[F0 + 2]), -1, ALIGN),
    (dict(n_features=2, features=[F0, F1 + 1], dims=[4, 4]), -1, ALIGN),
    (dict(type=None, weight=None), -3, None),
    (dict(n_edges=E31), -1, COUNT),
    (dict(n_edges=E31 - 1), -3, None),
    (dict(n_edges=E30, undirected=1), -1, COUNT),
    (dict(n_edges=E30 - 1, undirected=1), -3, None),
    # the order of the ladder: the earlier rule answers
    (dict(edges=False, out=False), -1, NULL),
    (dict(n_edges=-1, T=0, src=None), -1, NEG),
    (dict(T=0, n_node_types=40, src=None), -1, TYPES),
    (dict(n_node_types=40, src=None, nodes=None), -1, NTYPES),
    (dict(src=None, nodes=None), -1, ENDS),
    (dict(nodes=None, features=None), -1, FEAT_NODES),
    (dict(features=None, src=S + 1), -1, FEAT_NULL),
    (dict(dims=[0], src=S + 1, n_edges=E31), -1, FEAT_DIM),
    (dict(src=S + 1, n_edges=E31), -1, ALIGN),
]


def _answer_all():
    """(child) every row's call -> [[rc, last error], ...] on stdout"""
    spec = importlib.util.spec_from_file_location("_lib", os.path.join(ROOT, "euler_amd", "_lib.py"))
    _lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(_lib)             # (the binding alone: the package would import torch)
    L = _lib.lib()
    answers = []
    for changes, _, _ in ROWS:
        v = dict(BASE)
        v.update(changes)
        e = _lib.DevEdges()
        e.n_edges, e.n_nodes, e.n_edge_types, e.undirected = v["n_edges"], v["n_nodes"], v["T"], v["undirected"]
        e.src, e.dst, e.type, e.weight = v["src"], v["dst"], v["type"], v["weight"]
        e.nodes, e.node_type, e.node_weight = v["nodes"], v["node_type"], v["node_weight"]
        e.n_node_types, e.node_sampler, e.n_features = v["n_node_types"], v["node_sampler"], v["n_features"]
        keep = []
        if v["features"] is not None:
            ptrs = (C.c_void_p * len(v["features"]))(*v["features"])
            e.features = C.cast(ptrs, C.POINTER(C.c_void_p))
            keep.append(ptrs)
        if v["dims"] is not None:
            dims = (C.c_int32 * len(v["dims"]))(*v["dims"])
            e.feature_dims = C.cast(dims, _lib.i32p)
            keep.append(dims)
        h = C.c_void_p(0x1234)
        rc = L.euler_gpu_graph_create_from_edges(C.byref(e) if v["edges"] else None, 0, None,
                                                 C.byref(h) if v["out"] else None)
        answers.append([rc, L.euler_gpu_last_error().decode(), h.value])
    print(json.dumps(answers))


@pytest.fixture(scope="module")
def answers():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    return json.loads(run.stdout.decode().strip().splitlines()[-1])


def test_binding_matches_header():
    from euler_amd import _lib
    assert len(_lib.SIGNATURES["euler_gpu_graph_create_from_edges"][1]) == 4
    assert C.sizeof(_lib.DevEdges) == 2 * 8 + 2 * 4 + 7 * 8 + 4 * 4 + 2 * 8


@pytest.mark.parametrize("i", range(len(ROWS)), ids=lambda i: "%02d" % i)
def test_ladder_row(answers, i):
    changes, want_rc, want_text = ROWS[i]
    rc, text, handle = answers[i]
    assert rc == want_rc, (changes, rc, text)
    if want_rc == -1:
        assert text == want_text, changes
    if changes.get("out", True):
        assert handle is None, "no graph is returned on a failure"        # (*out = NULL)


if __name__ == "__main__":
    _answer_all()
