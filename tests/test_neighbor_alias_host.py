"""The alias neighbour mode on the host: the build of the tables and the draw
(euler_amd/csrc/nb_alias.h, nb_alias_draw.h) compiled with the host compiler
(tests/csrc/nb_alias_check.cc, -ffp-contract=off) against the numpy restatement
tests/neighbor_alias_ref.py - bit equality - and the restatement against the oracle's
AliasMethod::Init.  The same functions run once more as a stand-alone program built with
-fsanitize=address,undefined, on the same cases.  CPU only."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import neighbor_alias_ref as ref     # noqa: E402
import sampling_stats as S           # noqa: E402
from conftest import GOLDEN, load_csr     # noqa: E402

F = np.float32
f32p, i32p, i64p, u64p, u8p = (C.POINTER(t) for t in (C.c_float, C.c_int32, C.c_int64, C.c_uint64, C.c_uint8))
ENTRY = np.dtype([("id_self", "<u8"), ("id_alias", "<u8"), ("prob", "<f4"), ("w_self", "<f4"), ("w_alias", "<f4"),
                  ("pad", "<u4")])
assert ENTRY.itemsize == 32


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


def _build(out, flags):
    """tests/csrc/nb_alias_check.cc as host C++ (the headers it includes pull in the HIP runtime's
    host declarations, so the compiler is hipcc; a .cc file is compiled for the host alone)."""
    src = os.path.join(HERE, "csrc", "nb_alias_check.cc")
    inc = os.path.join(ROOT, "euler_amd", "csrc")
    deps = [src] + [os.path.join(inc, h) for h in ("nb_alias.h", "nb_alias_draw.h", "device_fns.h", "philox.h",
                                                   "common.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call([_hipcc(), "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", "-I" + inc,
                               "-I" + os.path.join(ROOT, "include")] + flags + [src, "-o", out])
    return out


@pytest.fixture(scope="module")
def NB():
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    L = C.CDLL(_build(os.path.join(out_dir, "libnb_alias_check.so"), ["-fPIC", "-shared"]))
    L.nba_alias_init.argtypes = [f32p, C.c_int64, f32p, i64p]
    L.nba_fixup.argtypes = [f32p, f32p, i64p, C.c_int64]
    L.nba_fixup.restype = C.c_int64
    L.nba_build.argtypes = [C.c_int64, C.c_int32, i64p, i32p, u64p, f32p, C.c_void_p]
    L.nba_draw.argtypes = [C.c_int64, C.c_int32, u64p, i64p, i32p, f32p, u64p, f32p, C.c_void_p, C.c_uint64,
                           C.c_uint32, u64p, C.c_int64, i32p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, u64p,
                           f32p, i32p, u8p]
    return L


def _p(a, t):
    return a.ctypes.data_as(t)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def host_build(L, csr):
    E = len(csr.nbr)
    tab = np.zeros(E + 1, ENTRY)
    nbr = np.concatenate([csr.nbr, np.zeros(1, np.uint64)])
    pw = np.concatenate([csr.prefix_w, np.zeros(1, F)])
    L.nba_build(csr.n_rows, csr.n_types, _p(csr.row_ptr, i64p), _p(csr.type_end, i32p), _p(nbr, u64p), _p(pw, f32p),
                tab.ctypes.data)
    return tab[:E]


def assert_tables_equal(tab, T, what=""):
    """entries (structured array or the export's arrays) == the restatement, bit for bit"""
    for name, want in (("id_self", T.id_self), ("id_alias", T.id_alias), ("prob", T.prob), ("w_self", T.w_self),
                       ("w_alias", T.w_alias)):
        got = np.ascontiguousarray(tab[name])
        assert np.array_equal(bits(got), bits(want)), (what, name, np.nonzero(bits(got) != bits(want))[0][:8])
    assert not tab["pad"].any()


# ------------------------------------------------------------------ the cases
class _G:
    """One-row-per-group-list graph in oracle.CSR's fields (no oracle needed)."""

    def __init__(self, rows, T=1, ids=None):
        """rows: per row a list of T weight lists"""
        self.n_types, self.n_rows = T, len(rows)
        self.row_id = np.asarray(ids if ids is not None else np.arange(1, len(rows) + 1), np.uint64)
        ptr, te, tp, pw, nbr = [0], [], [], [], []
        for r, groups in enumerate(rows):
            s, ts, cnt = F(0), F(0), 0
            for g in groups:
                tw = F(0)
                for x in np.asarray(g, F):
                    s, tw = F(s + x), F(tw + x)
                    pw.append(s)
                    nbr.append(1000 * (r + 1) + cnt)
                    cnt += 1
                ts = F(ts + tw)
                te.append(cnt)
                tp.append(ts)
            ptr.append(len(pw))
        self.row_ptr = np.asarray(ptr, np.int64)
        self.type_end = np.asarray(te, np.int32)
        self.type_prefix = np.asarray(tp, F)
        self.prefix_w = np.asarray(pw, F)
        self.nbr = np.asarray(nbr, np.uint64)


def _motif_graph(name):
    m = S.motif_of(name)
    rows = [[m.w[m.seg[j * m.T + t]:m.seg[j * m.T + t + 1]] for t in range(m.T)] for j in range(m.M)]
    if name == "hub":
        rows = rows[:4]         # the hub, the two rows of 600, one short row
    return _G(rows, m.T)


def _edge_graph():
    rng = np.random.default_rng(77)
    return _G([[[2.5]], [[1.0, 3.0]], [[0.0, 1.0]], [[4.0] * 7], [[0, 0, 3, 1, 2, 0, 5, 0]], [[0.0, 0.0, 0.0]],
               [[]], [(rng.random(33) * 7.5).astype(F)], [[1e-30, 1.0, 1e30]]])


def _pareto_graph():
    rng = np.random.default_rng(1611)
    return _G([[((rng.pareto(0.7, 1 << 16) + 1) * 0.5).astype(F)]])


def _golden(name):
    from oracle import oracle
    return load_csr(oracle, os.path.join(GOLDEN, name))


CASES = {
    "fixture": lambda: _golden("fixture_graph.npz"), "random": lambda: _golden("random_graph.npz"),
    "plain": lambda: _motif_graph("plain"), "typed": lambda: _motif_graph("typed"),
    "hub": lambda: _motif_graph("hub"), "uniform": lambda: _motif_graph("uniform"),
    "edges": _edge_graph, "pareto65536": _pareto_graph,
}
_BUILT = {}


def case(name):
    if name not in _BUILT:
        g = CASES[name]()
        _BUILT[name] = (g, ref.Tables(g))
    return _BUILT[name]


def groups_of(g):
    """(row, type, first flat edge, weights) of every group"""
    T = g.n_types
    for r in range(g.n_rows):
        b0 = int(g.row_ptr[r])
        w = ref.row_weights(g.prefix_w[b0:int(g.row_ptr[r + 1])])
        for t in range(T):
            b = 0 if t == 0 else int(g.type_end[r * T + t - 1])
            e = int(g.type_end[r * T + t])
            yield r, t, b0 + b, w[b:e]


# ------------------------------------------------------------------ build
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_oracles_alias_init(O, name):
    """(prob, alias) of the restatement == oracle.alias_init(norm) in every entry, except the
    entries the fix-up changed, which are listed; those have weight 0 and prob 1 in the oracle's."""
    g, T = case(name)
    changed = set(T.changed)
    for r, t, first, w in groups_of(g):
        if not T.has_table[r * g.n_types + t]:
            assert len(w) == 0 or ref.normalise(w)[0] == 0
            continue
        prob, alias = O.alias_init(ref.normalise(w)[1])
        for i in range(len(w)):
            if first + i in changed:
                assert w[i] == 0 and prob[i] == 1.0 and T.prob[first + i] == 0
            else:
                assert bits(prob[i:i + 1])[0] == bits(T.prob[first + i:first + i + 1])[0]
                assert alias[i] == T.alias_idx[first + i]
    print("%s: %d entries changed by the fix-up: %s" % (name, len(changed), sorted(changed)[:16]))


@pytest.mark.parametrize("name", list(CASES))
def test_host_build_equals_the_restatement(NB, name):
    g, T = case(name)
    assert_tables_equal(host_build(NB, g), T, name)


def test_shared_build_is_the_node_samplers(NB, O):
    """AliasBuild over plain arrays - what graph_build.hip's samplers call - == the oracle's"""
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 17, 1000):
        for w in (rng.random(n), np.ones(n), rng.pareto(0.7, n) + 1):
            norm = ref.normalise(w.astype(F))[1]
            prob, alias = np.zeros(n, F), np.zeros(n, np.int64)
            NB.nba_alias_init(_p(norm, f32p), n, _p(prob, f32p), _p(alias, i64p))
            want = O.alias_init(norm)
            assert np.array_equal(bits(prob), bits(want[0])) and np.array_equal(alias, want[1])


def _fix_both(NB, w, prob, alias):
    w = np.asarray(w, F)
    p1, a1 = np.asarray(prob, F).copy(), np.asarray(alias, np.int64).copy()
    p2, a2 = p1.copy(), a1.copy()
    changed = ref.fixup(w, p1, a1)
    n = NB.nba_fixup(_p(w, f32p), _p(p2, f32p), _p(a2, i64p), len(w))
    assert n == len(changed) and np.array_equal(bits(p1), bits(p2)) and np.array_equal(a1, a2)
    return p1, a1, changed


def test_fixup_alone(NB):
    """A hand-made table with a zero-weight leftover at prob 1.0 (what the drain loops leave when
    rounding empties the large stack early), and whatever a seeded search over 10^4 random groups of
    <= 16 f32 weights turns up."""
    w = [0.0, 2.0, 5.0, 5.0, 0.0, 1.0]
    prob = [1.0, 0.5, 1.0, 1.0, 0.0, 0.25]
    alias = [0, 2, 0, 0, 3, 2]
    p, a, changed = _fix_both(NB, w, prob, alias)
    assert changed == [0] and p[0] == 0 and a[0] == 2            # the FIRST of the two heaviest
    assert p[4] == 0 and a[4] == 3 and list(p[1:4]) == [0.5, 1.0, 1.0]      # nothing else moved
    rng = np.random.default_rng(20260)
    found = 0
    for _ in range(10000):
        d = int(rng.integers(1, 17))
        w = (rng.random(d) * 10.0 ** rng.integers(-6, 7, d)).astype(F)
        w[rng.random(d) < 0.3] = 0
        S_, norm = ref.normalise(w)
        if S_ == 0:
            continue
        prob, alias = ref.alias_init(norm)
        p, a, changed = _fix_both(NB, w, prob, alias)
        found += len(changed) > 0
        assert not ((w == 0) & (p != 0)).any()
    print("seeded search: %d of 10000 groups needed the fix-up" % found)


@pytest.mark.parametrize("name", list(CASES))
def test_table_mass_is_exact_within_the_derived_bound(name):
    """Without sampling: q_i (what the table draws, float64) is 0 exactly where w_i is 0 and within
    neighbor_alias_ref.mass_bound(d) of w_i / sum(w) - a bound from the count of f32 roundings in
    the build, stated there, not fitted to what comes out."""
    g, T = case(name)
    worst = 0.0
    for r, t, first, w in groups_of(g):
        if not T.has_table[r * g.n_types + t]:
            continue
        d = len(w)
        q = ref.table_mass(T.prob[first:first + d], T.alias_idx[first:first + d])
        p = w.astype(np.float64) / w.astype(np.float64).sum()
        assert (q[w == 0] == 0).all(), (name, r, t)
        assert abs(q.sum() - 1) < 1e-9
        err = np.abs(q - p).max()
        assert err <= ref.mass_bound(d), (name, r, t, d, err, ref.mass_bound(d))
        worst = max(worst, err / ref.mass_bound(d))
    print("%s: largest |q - p| / bound = %.3g" % (name, worst))


def test_noncentrality_of_the_tables_at_the_gpu_tests_sizes():
    """What tests/test_neighbor_alias_gpu.py's distribution cases would see of a CORRECT table's
    rounding: N sum (q - p)^2 / p per motif row at N = 8.4 M draws, against the exact model p.  A
    level-1e-7 test needs a noncentrality of tens to notice (sampling_stats.lambda_needed: 100 and
    more for power); these are asserted below 0.01."""
    N = S.R_GPU * 64 * 4
    worst = 0.0
    for name in ("plain", "typed", "uniform", "hub"):
        g, T = case(name)
        for r, t, first, w in groups_of(g):
            if not T.has_table[r * g.n_types + t]:
                continue
            d = len(w)
            q = ref.table_mass(T.prob[first:first + d], T.alias_idx[first:first + d])
            pw = g.prefix_w[int(g.row_ptr[r]):int(g.row_ptr[r + 1])].astype(np.float64)
            b = first - int(g.row_ptr[r])
            lo = 0.0 if b == 0 else pw[b - 1]
            p = np.diff(np.concatenate([[lo], pw[b:b + d]])) / (pw[b + d - 1] - lo)      # the exact mode's model
            if d > 2000:
                cells = S.equal_mass_bins(p[p > 0], S.HUB_BINS)
                lam = S.noncentrality(np.bincount(cells, weights=p[p > 0]), np.bincount(cells, weights=q[p > 0]), N)
            else:
                lam = S.noncentrality(p, q, N)
            worst = max(worst, lam)
            assert lam < 0.01, (name, r, t, lam)
    print("largest noncentrality at N = %d: %.3g" % (N, worst))


# ------------------------------------------------------------------ draw
def host_draw(L, g, tab, seed, call_id, roots, et, count, layout, default_node=-1):
    roots = np.ascontiguousarray(roots, np.uint64)
    n = len(roots)
    etv = np.zeros(32, np.int32)
    etv[:len(et)] = et
    ids, w = np.zeros(n * count + 1, np.uint64), np.zeros(n * count + 1, F)
    t, mask = np.zeros(n * count + 1, np.int32), np.zeros(n + 1, np.uint8)
    nbr = np.concatenate([g.nbr, np.zeros(1, np.uint64)])
    pw = np.concatenate([g.prefix_w, np.zeros(1, F)])
    tab = np.concatenate([tab, np.zeros(1, ENTRY)])
    L.nba_draw(g.n_rows, g.n_types, _p(g.row_id, u64p), _p(g.row_ptr, i64p), _p(g.type_end, i32p),
               _p(g.type_prefix, f32p), _p(nbr, u64p), _p(pw, f32p), tab.ctypes.data, seed, call_id, _p(roots, u64p), n,
               _p(etv, i32p), len(et), count, 1 if layout == "tf" else 0, default_node, _p(ids, u64p), _p(w, f32p),
               _p(t, i32p), _p(mask, u8p))
    return ids[:n * count].reshape(n, count), w[:n * count].reshape(n, count), t[:n * count].reshape(n, count), mask[:n]


def draw_cases(g):
    """(edge types, count, layout, roots): the three type modes, both layouts, unknown ids, invalid
    types"""
    T = g.n_types
    roots = np.concatenate([g.row_id[:40], [np.uint64(0), np.uint64(2 ** 40 + 3)], g.row_id[:3]])
    out = []
    for layout in ("tf", "core"):
        out += [([0], 5, layout, roots), ([T - 1], 4, layout, roots), ([], 7, layout, roots),
                (list(range(T)) + [0], 3, layout, roots), ([T], 3, layout, roots), ([-1], 2, layout, roots)]
        if T > 2:
            out += [([2, 0], 6, layout, roots), ([1, T], 2, layout, roots)]
    return out


@pytest.mark.parametrize("name", ["fixture", "random", "typed"])
def test_host_draw_equals_the_restatement(NB, O, name):
    g, T = case(name)
    tab = host_build(NB, g)
    for c, (et, count, layout, roots) in enumerate(draw_cases(g)):
        got = host_draw(NB, g, tab, 0xABCDEF12345, 40 + c, roots, et, count, layout, -1)
        want = ref.sample_neighbor(T, O, 0xABCDEF12345, 40 + c, roots, et, count, layout, -1)
        for a, b, what in zip(got, want, ("ids", "weights", "types", "mask")):
            assert np.array_equal(bits(a), bits(b)), (name, et, count, layout, what)


# ------------------------------------------------------------------ the sanitizer build
def _shadow_room():
    """In the child: the data-segment limit back at its hard value.  tests/conftest.py lowers the
    soft one for the test process; AddressSanitizer reserves (does not touch) terabytes of shadow."""
    import resource
    _, hard = resource.getrlimit(resource.RLIMIT_DATA)
    resource.setrlimit(resource.RLIMIT_DATA, (hard, hard))


def test_stand_alone_program_under_sanitizers(O, tmp_path):
    """The same functions as a program of its own, built -fsanitize=address,undefined, on the same
    cases: every graph above and the draw cases of the fixture, typed and random graphs.  Its output
    must be the restatement's bits and the sanitizers must stay silent."""
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = _build(os.path.join(out_dir, "nb_alias_check_san"),
                 ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    for name in CASES:
        g, T = case(name)
        calls = draw_cases(g) if name in ("fixture", "random", "typed") else []
        E = len(g.nbr)
        blob = [struct.pack("<3q", g.n_rows, g.n_types, len(calls)), g.row_id.astype("<u8").tobytes(),
                g.row_ptr.astype("<i8").tobytes(), g.type_end.astype("<i4").tobytes(),
                g.type_prefix.astype("<f4").tobytes(), g.nbr.astype("<u8").tobytes(),
                g.prefix_w.astype("<f4").tobytes()]
        for c, (et, count, layout, roots) in enumerate(calls):
            etv = np.zeros(32, "<i4")
            etv[:len(et)] = et
            blob += [struct.pack("<Q6q", 0xABCDEF12345, 40 + c, len(et), count, 1 if layout == "tf" else 0, -1,
                                 len(roots)), etv.tobytes(), np.asarray(roots, "<u8").tobytes()]
        fin, fout = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        with open(fin, "wb") as f:
            f.write(b"".join(blob))
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, preexec_fn=_shadow_room)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stdout, r.stderr[-2000:])
        raw = open(fout, "rb").read()
        assert_tables_equal(np.frombuffer(raw[:32 * E], ENTRY), T, name)
        off = 32 * E
        for c, (et, count, layout, roots) in enumerate(calls):
            want = ref.sample_neighbor(T, O, 0xABCDEF12345, 40 + c, roots, et, count, layout, -1)
            for b, dt in zip(want, ("<u8", "<f4", "<i4", "u1")):
                nbytes = b.size * np.dtype(dt).itemsize
                got = np.frombuffer(raw[off:off + nbytes], dt).reshape(b.shape)
                assert np.array_equal(bits(got), bits(b)), (name, c)
                off += nbytes
        assert off == len(raw)
