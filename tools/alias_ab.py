"""A/B of the two neighbour draws in ONE process: the exact mode's [25, 10] fanout step against the
alias mode's on the same graph, alternated, device events around --steps steps each, repeated
--repeats times for the spread; the build time and bytes of the alias tables.  Two graphs: the
benchmark's metric graph (synthetic, 100 M nodes / 1 B edges) and a heavy-tailed one (Pareto 0.7
weights, built on the host: the synthetic generator has no such weights, so it is smaller).

  python tools/alias_ab.py                                    # both graphs, JSON lines
  python tools/alias_ab.py --graphs heavy --heavy-nodes 2000000
  python tools/alias_ab.py --trace [--graphs metric]          # a run of its own under
        rocprofv3 --kernel-trace --stats (kernel time of both modes' kernels and of the build)
  python tools/alias_ab.py --pmc TCC_EA0_RDREQ_sum [--graphs metric]   # a run of its own under rocprofv3 --pmc
        (read requests per launch, the counter of DESIGN 4.2; never collected together with a trace)
The profiler runs start this script again as a fresh child with few steps."""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FAN = [25, 10]


def heavy_graph(euler_amd, np, nodes, degree):
    rng = np.random.default_rng(11)
    E = nodes * degree
    w = ((rng.pareto(0.7, E) + 1) * 0.5).astype(np.float32).reshape(nodes, degree)
    prefix = np.cumsum(w, axis=1, dtype=np.float32)
    return euler_amd.Graph.from_csr(np.arange(1, nodes + 1, dtype=np.uint64), np.arange(nodes + 1, dtype=np.int64) * degree,
                                    np.full(nodes, degree, np.int32), rng.integers(1, nodes + 1, E).astype(np.uint64),
                                    prefix.reshape(-1), prefix[:, -1].copy(), 1)


def measure(a, name):
    import numpy as np
    import torch
    import euler_amd
    t0 = time.perf_counter()
    if name == "metric":
        n = a.nodes
        G = euler_amd.Graph.synthetic(euler_amd.synth_params(20240521, a.nodes, a.edges, weighted=True))
    else:
        n = a.heavy_nodes
        G = heavy_graph(euler_amd, np, a.heavy_nodes, a.heavy_degree)
    torch.cuda.synchronize()
    res = {"graph": name, "nodes": n, "edges": G.num_edges, "batch": a.batch, "steps": a.steps,
           "graph_s": round(time.perf_counter() - t0, 2), "flat_bytes": G.device_bytes}
    G.set_seed(20240521)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    roots = torch.randint(1, n + 1, (24, a.batch), generator=gen, device="cuda")

    def step(i, method):
        return G.sample_fanout(roots[i % 24], [[0], [0]], FAN, n + 1, call_id=2 * i, method=method)

    t1 = time.perf_counter()
    G.build_neighbor_alias()                         # returns when the build has finished
    res["alias_build_s"] = round(time.perf_counter() - t1, 4)
    res["alias_bytes"], res["alias_entries"] = G.neighbor_alias()
    step(0, "exact")                                 # builds the exact mode's indexes
    torch.cuda.synchronize()
    res["exact_index_bytes"] = G.device_bytes - res["flat_bytes"] - res["alias_bytes"]
    if name == "heavy":
        res["index_overflow_rows"] = int(len(G.index_overflow_rows()))
    for i in range(24):
        step(i, "exact")
        step(i, "alias")
    ms = {"exact": [], "alias": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(a.repeats):
        for method in ("exact", "alias"):
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(a.steps):
                step(i, method)
            ev[1].record()
            torch.cuda.synchronize()
            ms[method].append(round(ev[0].elapsed_time(ev[1]) / a.steps, 4))
    res["ms_per_step"] = ms
    print(json.dumps(res), flush=True)
    G.close()


def profiled(a, extra, pattern):
    """this script again, as a fresh child under rocprofv3; prints the rows of its CSVs that name a
    sampling or build kernel"""
    out = tempfile.mkdtemp(prefix="alias_ab_")
    cmd = ["rocprofv3"] + extra + ["-d", out, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                                   "--graphs", a.graphs, "--steps", "20", "--repeats", "1", "--nodes", str(a.nodes),
                                   "--edges", str(a.edges), "--heavy-nodes", str(a.heavy_nodes), "--heavy-degree",
                                   str(a.heavy_degree), "--batch", str(a.batch)]
    print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, timeout=a.child_timeout)
    for f in sorted(glob.glob(os.path.join(out, "**", pattern), recursive=True)):
        print("==", f)
        shown = 0
        with open(f) as fh:
            for i, line in enumerate(fh):
                if i == 0 or (shown < a.rows and any(k in line for k in ("Alias", "Fanout", "SampleNeighbor", "Dedup"))):
                    print(line.rstrip()[:400])
                    shown += i > 0
    return r.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="metric,heavy")
    ap.add_argument("--nodes", type=int, default=100_000_000)
    ap.add_argument("--edges", type=int, default=1_000_000_000)
    ap.add_argument("--heavy-nodes", type=int, default=2_000_000)
    ap.add_argument("--heavy-degree", type=int, default=50)
    ap.add_argument("--batch", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--pmc", default="")
    ap.add_argument("--child-timeout", type=int, default=900)
    ap.add_argument("--rows", type=int, default=60, help="rows shown per profiler CSV")
    a = ap.parse_args()
    if a.trace:
        return profiled(a, ["--kernel-trace", "--stats"], "*stats*.csv")
    if a.pmc:
        return profiled(a, ["--pmc", a.pmc], "*counter*.csv")
    for name in a.graphs.split(","):
        measure(a, name)
    return 0


if __name__ == "__main__":
    sys.exit(main())
