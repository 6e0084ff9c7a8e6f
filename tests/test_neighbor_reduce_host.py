"""The arithmetic of the full-neighbour aggregation (euler_amd/csrc/mp_rows.h), compiled with the
host compiler, against the numpy restatement tests/neighbor_reduce_ref.py - bit equality unless a
bound is stated - and the argument ladders of euler_gpu_neighbor_reduce / euler_gpu_neighbor_degree
through the C ABI in a child process that sees no GPU: return code and the full last-error text of
every call that breaks one rule, as tests/test_fp8_entry_args_host.py does.  The ladders are host
arithmetic in front of the first HIP call, so the pointers - the graph handle among them - are
made-up addresses nothing dereferences.  CPU only."""
import ctypes as C
import importlib.util
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import neighbor_reduce_ref as ref     # noqa: E402

f32p, i32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
MODE = {"add": 0, "max": 1, "mean": 2}
KIND = {None: 0, "edge": 1, "norm": 2}
U = 2.0 ** -24
F = np.float32

NEW_SYMBOLS = ["euler_gpu_neighbor_reduce", "euler_gpu_neighbor_degree"]


def _cxx():
    return shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _build(out, flags):
    src = os.path.join(HERE, "csrc", "neighbor_reduce_check.cc")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", h) for h in ("mp_rows.h", "mp_gcn.h", "mp_weighted.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        # -ffp-contract=off: the host build may not fuse a product and a sum either
        subprocess.check_call([_cxx(), "-O2", "-std=c++17", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "euler_amd", "csrc")] + flags + [src, "-o", out])
    return out


@pytest.fixture(scope="module")
def NR():
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    L = C.CDLL(_build(os.path.join(out_dir, "libneighbor_reduce_check.so"), ["-fPIC", "-shared"]))
    L.neighbor_reduce_row.argtypes = [C.c_int, C.c_int, C.c_int, f32p, C.c_int64, C.c_int64, u64p, f32p, i32p,
                                      C.c_int32, i32p, C.c_int32, C.c_int, C.c_uint64, C.c_float, f32p, f32p,
                                      C.c_float, C.c_float, f32p]
    L.neighbor_reduce_row.restype = C.c_int
    L.neighbor_listed_degree.argtypes = [i32p, C.c_int32, i32p, C.c_int32, C.c_int]
    L.neighbor_listed_degree.restype = C.c_int64
    return L


def same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


def one_row_graph(rng, lens, node=5, rows=23):
    """a graph of ONE row (id `node`) whose groups have the given lengths: ids in [0, rows + 3) -
    some past the table -, one with high bits set, non-trivial running sums"""
    e = int(sum(lens))
    nbr = rng.integers(0, rows + 3, e).astype(np.uint64)
    if e:
        nbr[0] |= np.uint64(7 << 32)
    w = (rng.random(e) * 3 + 0.01).astype(F)
    prefix = np.cumsum(w, dtype=F) if e else np.zeros(0, F)
    type_end = np.cumsum(lens).astype(np.int32)
    return ref.Rows([node], [0, e], type_end, nbr, prefix, len(lens))


def host_row(L, G, op, kind, lane_cols, x, edge_types, self_loop, node, nd, norm_src, root=None, a=1.0, b=1.0,
             has_row=True):
    x = np.ascontiguousarray(x, F)
    et = np.ascontiguousarray(edge_types, np.int32)
    ns = np.ascontiguousarray(norm_src, F)
    rt = None if root is None else np.ascontiguousarray(root, F)
    out = np.full(x.shape[1], np.nan, F)
    nbr = np.concatenate([G.nbr, np.zeros(1, np.uint64)])          # (never empty: a valid pointer)
    pw = np.concatenate([G.prefix_w, np.zeros(1, F)])
    te = np.ascontiguousarray(G.type_end[0])
    rc = L.neighbor_reduce_row(MODE[op], KIND[kind], lane_cols, x.ctypes.data_as(f32p), x.shape[1], x.shape[0],
                               nbr.ctypes.data_as(u64p), pw.ctypes.data_as(f32p),
                               te.ctypes.data_as(i32p) if has_row else None, G.T, et.ctypes.data_as(i32p), et.size,
                               int(self_loop), node, float(nd), ns.ctypes.data_as(f32p),
                               rt.ctypes.data_as(f32p) if rt is not None else None, float(a), float(b),
                               out.ctypes.data_as(f32p))
    assert rc == 0
    return out


@pytest.mark.parametrize("op", ["add", "max", "mean"])
@pytest.mark.parametrize("listed", [0, 1, 7, 8, 9, 12, 13, 65])        # the batch ladder 8 / 4 / 1
def test_row_function_equals_the_numpy_loop(NR, op, listed):
    rng = np.random.default_rng(2000 + listed)
    rows, d, node = 23, 8, 5
    G = one_row_graph(rng, [3, listed, 2])
    x = ((rng.random((rows, d)) * 8 - 4) * 10.0 ** rng.integers(-3, 4, (rows, d))).astype(F)
    norm_src = ref.norm_of(rng.integers(0, 50, rows))
    nd = ref.norm_of(np.array([listed + 1]))
    root = (rng.random((1, d)) * 6 - 3).astype(F)
    for kind in (None, "edge", "norm"):
        for self_loop in (False, True):
            want = ref.aggregate(G, op, x, [node], [1], kind, (nd, norm_src), self_loop)
            assert want.shape == (1, d)
            for lanes in (1, 4, 8):
                got = host_row(NR, G, op, kind, lanes, x, [1], self_loop, node, nd[0], norm_src)
                assert same(got, want[0]), (kind, self_loop, lanes)
            for a, b in ((F(1 - 0.1), F(0.1)), (1.0, 1.0)):
                got = host_row(NR, G, op, kind, 4, x, [1], self_loop, node, nd[0], norm_src, root[0], a, b)
                assert same(got, ref.aggregate(G, op, x, [node], [1], kind, (nd, norm_src), self_loop, root, a, b)[0])
    if listed == 0:
        empty = host_row(NR, G, op, None, 1, x, [1], False, node, 0, norm_src)
        assert same(empty, np.full(d, -1e9 if op == "max" else 0, F))


def test_type_lists_follow_get_full_neighbor(NR):
    """groups in listed order, a type listed twice read twice, a type outside [0, T) skipped, a
    node without a row: only its self update"""
    rng = np.random.default_rng(3)
    G = one_row_graph(rng, [9, 4, 13])
    x = (rng.random((23, 4)) - 0.5).astype(F)
    ns = ref.norm_of(np.arange(23))
    for et in ([0], [2, 0], [1, 1], [0, 7], [-1, 2], [0, 1, 2], []):
        for kind in (None, "edge"):
            want = ref.aggregate(G, "add", x, [5], et, kind)[0]
            assert same(host_row(NR, G, "add", kind, 4, x, et, False, 5, 0, ns), want), et
        te = np.ascontiguousarray(G.type_end[0])
        e32 = np.ascontiguousarray(et, np.int32)
        deg = NR.neighbor_listed_degree(te.ctypes.data_as(i32p), 3, e32.ctypes.data_as(i32p), e32.size, 1)
        assert deg == ref.degree(G, [5], et, True)[0]
    want = ref.aggregate(G, "mean", x, [99], [0, 1, 2], None, None, True)[0]          # 99 has no row
    got = host_row(NR, G, "mean", None, 1, x, [0, 1, 2], True, 99, 0, ns, has_row=False)
    assert same(got, want) and same(want, (x[22] / F(F(1) + F(1e-7))).astype(F))         # clamped to the last row
    e32 = np.array([0, 1], np.int32)
    assert NR.neighbor_listed_degree(None, 3, e32.ctypes.data_as(i32p), 2, 0) == 0


def test_product_and_sum_are_two_roundings_not_an_fma(NR):
    """x * w = 1 + 2^-11 + 2^-24 exactly; rounded to fp32 it is 1 + 2^-11 (a tie, to even), and
    adding it to acc = -(1 + 2^-11) gives 0.  A fused multiply-add keeps the 2^-24."""
    x = F(1 + 2.0 ** -12)
    w = F(1 + 2.0 ** -12)
    acc = F(-(1 + 2.0 ** -11))
    two_step = F(F(x * w) + acc)
    fused = F(np.float64(x) * np.float64(w) + np.float64(acc))
    assert two_step == 0 and fused == F(2.0 ** -24) and two_step != fused
    # the row: first acc's table row with edge weight 1, then x's with edge weight w
    table = np.array([[acc] * 4, [x] * 4], F)
    G = ref.Rows([5], [0, 2], [2], [0, 1], np.array([1.0, F(1.0) + w], F), 1)
    assert G.edge_weight(0, 1) == w
    for lanes in (1, 4):
        got = host_row(NR, G, "add", "edge", lanes, table, [0], False, 5, 0, [1, 1])
        assert same(got, np.zeros(4, F)), lanes
        assert same(got, ref.aggregate(G, "add", table, [5], [0], "edge")[0])


def test_edge_weights_are_row_absolute_prefix_differences(NR):
    """w(p) = fl(prefix[p] - prefix[p - 1]) with p counted in the whole row: the first entry of the
    SECOND group subtracts the last running sum of the first group, not 0"""
    prefix = np.array([0.5, 1.75, 4.0, 4.125, 10.0], F)
    G = ref.Rows([5], [0, 5], [2, 5], [0, 1, 2, 3, 4], prefix, 2)
    x = np.eye(5, dtype=F)                        # out[c] = the weight of the entry that names row c
    got = host_row(NR, G, "add", "edge", 1, x, [1], False, 5, 0, np.ones(5))
    assert same(got, np.array([0, 0, F(4.0) - F(1.75), F(4.125) - F(4.0), F(10.0) - F(4.125)], F))
    got = host_row(NR, G, "add", "edge", 1, x, [1, 0], False, 5, 0, np.ones(5))
    assert same(got, np.array([0.5, F(1.75) - F(0.5), 2.25, 0.125, 5.875], F))
    assert same(got, ref.aggregate(G, "add", x, [5], [1, 0], "edge")[0])


@pytest.mark.parametrize("op", ["add", "mean"])
@pytest.mark.parametrize("kind", [None, "edge", "norm"])
def test_float64_bound(NR, op, kind):
    """|out - exact| <= gamma_(L + 1) * sum |terms|, gamma_k = k u / (1 - k u), u = 2^-24, exact in
    float64 from the same fp32 weights (a mean: and the same fp32 denominator): one rounding per
    message, L - 1 for the sum, one for a mean's divide - at most L + 1"""
    rng = np.random.default_rng(31)
    rows, d = 23, 8
    for listed in (1, 9, 65, 300):
        G = one_row_graph(rng, [listed, 5])
        x = ((rng.random((rows, d)) * 2 - 1) * 10.0 ** rng.integers(-2, 3, (rows, d))).astype(F)
        ns = ref.norm_of(rng.integers(1, 50, rows))
        nd = ref.norm_of(np.array([listed + 6]))
        got = host_row(NR, G, op, kind, 4, x, [0, 1], True, 5, nd[0], ns).astype(np.float64)
        ups = ref.updates(G, 0, 5, [0, 1], kind, (nd, ns), True, rows)
        want, scale = ref.exact_f64(op, x, ups)
        k = len(ups) + 1
        assert len(ups) == listed + 6
        assert np.all(np.abs(got - want) <= k * U / (1 - k * U) * scale)


def test_check_program_runs_on_its_own():
    """the same source as a program with its own main (the form a sanitizer build takes)"""
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = _build(os.path.join(out_dir, "neighbor_reduce_check"), [])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert run.returncode == 0 and run.stdout.decode().strip().endswith("ok"), run.stdout.decode()[-2000:]


# ---- the two argument ladders -------------------------------------------------------------------
GH, N_, T_, O_, ND, NS, R_, ET = 0x9000, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
BASE = dict(g=GH, mode=0, nodes=N_, n=4, et=ET, k=2, kind=0, self_loop=0, table=T_, dtype=0, rows=10, d=32,
            nd=None, ns=None, root=None, root_dtype=0, a=1.0, b=1.0, out=O_, out_dtype=0, as_norm=0)
ARGS = {
    "neighbor_reduce": ["g", None, "mode", "nodes", "n", "et", "k", "kind", "self_loop", "table", "dtype", "rows",
                        "d", "nd", "ns", "root", "root_dtype", "a", "b", "out", "out_dtype"],
    "neighbor_degree": ["g", None, "nodes", "n", "et", "k", "self_loop", "as_norm", "out"],
}
NRD, DEG = ("neighbor_reduce",), ("neighbor_degree",)
BOTH = NRD + DEG
CODES = " (0 fp32, 1 bf16, 2 fp16)"
E31 = 1 << 31
NORM = dict(kind=2, nd=ND, ns=NS)
ALIGN = "a buffer is not aligned to its type"
NORM_RULE = "norm_dst and norm_src come with weight_kind 2, and only with it"

ROWS = [
    (BOTH, dict(g=None), -4, "%s: null graph"),
    (NRD, dict(dtype=3), -1, "%s: unknown dtype 3" + CODES),
    (NRD, dict(dtype=-1), -1, "%s: unknown dtype -1" + CODES),
    (NRD, dict(out_dtype=1), -1, "%s: out_dtype 1 is neither fp32 nor the input's dtype"),
    (NRD, dict(dtype=1, out_dtype=2), -1, "%s: out_dtype 2 is neither fp32 nor the input's dtype"),
    (NRD, dict(root=R_, root_dtype=2), -1, "%s: root_dtype 2 is neither fp32 nor the input's dtype"),
    (NRD, dict(root_dtype=7, n=0), 0, None),                 # no root: its dtype is not looked at
    (NRD, dict(mode=-1), -1, "%s: mode is 0 add, 1 max, 2 mean"),
    (NRD, dict(mode=3), -1, "%s: mode is 0 add, 1 max, 2 mean"),
    (NRD, dict(kind=3), -1, "%s: weight_kind is 0 none, 1 edge, 2 norm"),
    (NRD, dict(kind=-1), -1, "%s: weight_kind is 0 none, 1 edge, 2 norm"),
    (BOTH, dict(n=-1), -1, "%s: bad shape"),
    (BOTH, dict(k=-1), -1, "%s: bad shape"),
    (NRD, dict(d=-1), -1, "%s: bad shape"),
    (BOTH, dict(n=0), 0, None),
    (NRD, dict(d=0), 0, None),
    (BOTH, dict(n=0, nodes=None, out=None, table=None, et=None), 0, None),
    (NRD, dict(d=0, k=33, rows=0), 0, None),
    (BOTH, dict(nodes=None), -1, "%s: null buffer"),
    (BOTH, dict(out=None), -1, "%s: null buffer"),
    (BOTH, dict(et=None), -1, "%s: null buffer"),
    (NRD, dict(table=None), -1, "%s: null buffer"),
    (BOTH, dict(k=33), -1, "%s: more than 32 listed edge types"),
    (NRD, dict(rows=0), -1, "%s: the table must have at least one row"),
    (NRD, dict(rows=-5), -1, "%s: the table must have at least one row"),
    (NRD, dict(rows=E31), -1, "%s: the table must have fewer than 2^31 rows"),
    (BOTH, dict(n=E31), -1, "%s: n >= 2^31"),
    (NRD, dict(kind=2), -1, "%s: " + NORM_RULE),
    (NRD, dict(kind=2, nd=ND), -1, "%s: " + NORM_RULE),
    (NRD, dict(kind=2, ns=NS), -1, "%s: " + NORM_RULE),
    (NRD, dict(kind=1, nd=ND, ns=NS), -1, "%s: " + NORM_RULE),
    (NRD, dict(kind=0, ns=NS), -1, "%s: " + NORM_RULE),
    (BOTH, dict(nodes=N_ + 4), -1, "%s: " + ALIGN),
    (BOTH, dict(out=O_ + 2), -1, "%s: " + ALIGN),
    (NRD, dict(table=T_ + 2), -1, "%s: " + ALIGN),
    (NRD, dict(dtype=1, table=T_ + 1), -1, "%s: " + ALIGN),
    (NRD, dict(dtype=2, out_dtype=2, out=O_ + 1), -1, "%s: " + ALIGN),
    (NRD, dict(root=R_ + 2), -1, "%s: " + ALIGN),
    (NRD, dict(dtype=1, root=R_ + 1, root_dtype=1), -1, "%s: " + ALIGN),
    (NRD, dict(NORM, nd=ND + 2), -1, "%s: " + ALIGN),
    (NRD, dict(NORM, ns=NS + 1), -1, "%s: " + ALIGN),
    # the order of the ladders: the earlier rule answers
    (NRD, dict(g=None, dtype=9), -4, "%s: null graph"),
    (NRD, dict(dtype=9, mode=9), -1, "%s: unknown dtype 9" + CODES),
    (NRD, dict(mode=9, kind=9), -1, "%s: mode is 0 add, 1 max, 2 mean"),
    (NRD, dict(kind=9, n=-1), -1, "%s: weight_kind is 0 none, 1 edge, 2 norm"),
    (BOTH, dict(n=-1, out=None), -1, "%s: bad shape"),
    (BOTH, dict(out=None, k=33), -1, "%s: null buffer"),
    (NRD, dict(k=33, rows=0), -1, "%s: more than 32 listed edge types"),
    (NRD, dict(rows=E31, n=E31), -1, "%s: the table must have fewer than 2^31 rows"),
    (NRD, dict(n=E31, kind=2), -1, "%s: n >= 2^31"),
    (DEG, dict(k=33, n=E31), -1, "%s: more than 32 listed edge types"),
    (DEG, dict(n=E31, out=O_ + 1), -1, "%s: n >= 2^31"),
    (NRD, dict(kind=2, out=O_ + 2), -1, "%s: " + NORM_RULE),
]


def _cases(row):
    out = []
    for entry in row[0]:
        v = dict(BASE)
        v.update(row[1])
        out.append((entry, [v[name] if name else None for name in ARGS[entry]]))
    return out


def _answer_all():
    """(child) every call of every row -> [[[rc, last error], ...], ...] on stdout"""
    spec = importlib.util.spec_from_file_location("_lib", os.path.join(ROOT, "euler_amd", "_lib.py"))
    _lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(_lib)             # (the binding alone: the package would import torch)
    L = _lib.lib()
    answers = []
    for row in ROWS:
        got = []
        for entry, values in _cases(row):
            rc = getattr(L, "euler_gpu_" + entry)(*values)
            got.append([rc, L.euler_gpu_last_error().decode()])
        answers.append(got)
    print(json.dumps(answers))


@pytest.fixture(scope="module")
def answers():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    return json.loads(run.stdout.decode().strip().splitlines()[-1])


def test_tables_cover_both_entries():
    assert sorted(ARGS) == sorted({e for row in ROWS for e in row[0]})
    from euler_amd import _lib
    for entry, names in ARGS.items():
        assert len(_lib.SIGNATURES["euler_gpu_" + entry][1]) == len(names), entry


@pytest.mark.parametrize("i", range(len(ROWS)), ids=lambda i: "%03d-%s" % (i, ROWS[i][0][0]))
def test_row(answers, i):
    row = ROWS[i]
    for (entry, values), (rc, text) in zip(_cases(row), answers[i]):
        assert rc == row[2], (entry, values, rc, text)
        if row[2] != 0:
            assert text == row[3] % entry, (entry, values)


def test_new_entries_are_exported_and_bound():
    from euler_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
        assert name + "(" in hdr, name


def test_new_files_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "euler_amd", "csrc", "Makefile")).read()
    assert "neighbor_reduce_kernels.hip" in mk and "mp_rows.h" in mk and "mp_loaders.h" in mk


if __name__ == "__main__":
    _answer_all()
