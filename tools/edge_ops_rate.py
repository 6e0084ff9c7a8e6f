"""Rates of the edge store's hot paths, one JSON line: a synthetic power-law graph of
>= 200M edge records built on the device (Graph.edges_from_rows) with a 16-float dense, a 2-value
uint64 and an 8-byte binary edge feature; then
  sample_edge   16M draws (one type, and type -1)
  lookup+dense  1M (src, dst, type) triples, 10 % of them misses, d = 16 fetched in the same kernel
  binary        the same triples' 8-byte binary feature (count pass + fill pass)
Every rate comes with its algorithmic bytes, frac of 8 TB/s, random 128-byte lines per item and
lines/s against the ~54 G lines/s this chip completes for random reads.
Environment: EO_NODES / EO_EDGES size the graph (defaults 25M / 240M CSR entries)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import euler_amd                      # noqa: E402

N = int(os.environ.get("EO_NODES", 25_000_000))
E = int(os.environ.get("EO_EDGES", 240_000_000))
PEAK_BPS, PEAK_LINES = 8e12, 54e9
REPS = 20


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps / 1e3      # seconds per call


def rate(items, secs, algo_bytes, lines_per_item):
    return {"items": items, "ms": round(secs * 1e3, 4), "items_per_s": items / secs,
            "algo_bytes": algo_bytes, "frac": round(algo_bytes / secs / PEAK_BPS, 4),
            "lines_per_item": lines_per_item,
            "lines_per_s": items * lines_per_item / secs,
            "lines_frac": round(items * lines_per_item / secs / PEAK_LINES, 4)}


def main():
    torch.cuda.set_device(0)
    out = {"tool": "edge_ops_rate"}
    p = euler_amd.synth_params(20240612, N, E, n_types=2, weighted=True)
    G = euler_amd.Graph.synthetic(p, device=0)
    bytes0 = G.device_bytes
    t = time.time()
    G.edges_from_rows()
    out["edges_from_rows_s"] = round(time.time() - t, 2)
    n = G.num_edge_records
    out["graph"] = "%d nodes / %d CSR entries, 2 edge types -> %d edge records" % (N, G.num_edges, n)
    out["store_bytes_per_record"] = round((G.device_bytes - bytes0) / n, 2)
    # features: column 0 of the dense row = the ordinal (checked below), the rest constant
    dense = np.empty((n, 16), np.float32)
    dense[:] = np.arange(16, dtype=np.float32)
    dense[:, 0] = np.arange(n).astype(np.float32)
    sparse = np.empty((n, 2), np.uint64)
    sparse[:] = np.array([7, 9], np.uint64)
    binary = np.empty((n, 8), np.uint8)
    binary[:] = np.frombuffer(b"edgebyte", np.uint8)
    t = time.time()
    G.set_edge_features(dense=[dense], sparse=[sparse], binary=[binary])
    out["set_edge_features_s"] = round(time.time() - t, 2)
    del dense, sparse, binary

    G.set_seed(1)
    D = 16 << 20
    rates = {}
    for name, ty in (("sample_edge_type0", 0), ("sample_edge_all", -1)):
        s = timed(lambda: G.sample_edge(D, ty, call_id=3))
        # per draw: 32-byte alias entry + 20 bytes of the slot read, 24 bytes written; the
        # alias entry and the slot are two random lines
        rates[name] = rate(D, s, D * (32 + 20 + 24), 2)

    Q = 1 << 20
    q = G.sample_edge(Q, -1, call_id=9)
    miss = torch.rand(Q, device=q.device) < 0.1
    q[:, 1] = torch.where(miss, -7 - torch.arange(Q, device=q.device), q[:, 1])
    q = q.contiguous()
    hits = int((~miss).sum())
    ords = G.edge_ordinals(q)
    d, = G.get_edge_dense_feature(q, [0], [16])
    torch.cuda.synchronize()
    assert torch.equal(ords < 0, miss), "lookup: misses differ"
    assert torch.equal(d[:, 0][~miss], ords[~miss].float()), "dense fetch: wrong rows"
    s = timed(lambda: G.edge_ordinals(q))
    rates["lookup"] = rate(Q, s, Q * (24 + 8) + hits * 32, 1)
    s = timed(lambda: G.get_edge_dense_feature(q, [0], [16]))
    # query 24 B, slot 32 B (hits), feature row 64 B (hits), output row 64 B; the slot's line and
    # the feature row's line per hit, one line per miss
    rates["lookup_dense16"] = rate(Q, s, Q * (24 + 64) + hits * (32 + 64),
                                   round((2 * hits + (Q - hits)) / Q, 3))
    (off, data), = G.get_edge_binary_feature(q, [0])
    torch.cuda.synchronize()
    assert int(off[-1]) == 8 * hits
    s = timed(lambda: G.get_edge_binary_feature(q, [0]))
    # two passes (count, fill), each a lookup; the fill reads 8 bytes of the row's line
    rates["binary"] = rate(Q, s, Q * (2 * 24 + 8 + 8) + hits * (2 * 32 + 8 + 8),
                           round((3 * hits + 2 * (Q - hits)) / Q, 3))
    out["rates"] = rates
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
