#!/usr/bin/env python3
"""Graph.from_edges against the host route it replaces, on one GPU.

    python tools/graph_from_edges_rate.py [--log2-edges 24 27] [--repeats 3] [--out FILE.json]

The graph: a power-law edge list generated on the device from a fixed seed (src = a cubed uniform
draw over N = E / 16 nodes, dst uniform), two edge types, fp32 weights in [0.5, 4.5), plus one hub row
of 2^20 entries.  Per size, wall clock around each route with a device synchronisation before and
after, `--repeats` runs each, alternating the routes; the median is reported and every run is listed.
One run of each route is made first and not counted (code objects, allocator pools).

  route (a)  what the library offered these inputs before: copy the edge list to the host, numpy
             stable argsort by (row, type), Node::Init's running sums (the C restatement of the
             oracle when it is built, else a numpy cumsum per row), Graph.from_csr.
  route (b)  Graph.from_edges.

Also reported for (b): its passes' times (Graph.from_edges_pass_ms, the stream drained after each);
the peak of the device's used bytes above the level before the call, polled from another thread every
millisecond (hipMemGetInfo: device-wide, so other tenants' allocations would show in it) - the
library's temporaries come from hipMalloc, which torch.cuda.max_memory_allocated does not see; that
counter's rise is printed next to it; and the long rows' prefix pass alone on a graph that is only
the hub row.  A run without a GPU fails: nothing here falls back."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import euler_amd                                   # noqa: E402

HUB = 1 << 20
SUMS = ""               # which Node::Init the host route ran: recorded in every result line
T = 2


def make_edges(log2_e, seed=20240607):
    e = 1 << log2_e
    n = max(e // 16, 64)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand(e, device="cuda", generator=gen, dtype=torch.float64)
    src = (u * u * u * n).long().clamp_(0, n - 2) + 1                  # 1 .. n - 1, heavy at the low ids
    dst = torch.randint(1, n + 1, (e,), device="cuda", generator=gen)
    hub = min(HUB, e // 4)
    src[torch.arange(hub, device="cuda") * (e // hub)] = n             # the hub: id n, spread over the list
    typ = torch.randint(0, T, (e,), device="cuda", generator=gen, dtype=torch.int32)
    w = torch.rand(e, device="cuda", generator=gen) * 4 + 0.5
    return n, src, dst, typ, w


def route_host(n, src, dst, typ, w):
    s, d, t, ww = src.cpu().numpy(), dst.cpu().numpy().astype(np.uint64), typ.cpu().numpy(), w.cpu().numpy()
    key = (s - 1) * T + t
    order = np.argsort(key, kind="stable")
    seg = np.searchsorted(key[order], np.arange(n * T + 1)).astype(np.int64)
    nbr, raw = d[order], ww[order]
    row_id = np.arange(1, n + 1, dtype=np.uint64)
    try:
        from oracle import oracle as O
        O.lib()
    except (ImportError, OSError):
        O = None
    global SUMS
    if O is not None:
        SUMS = "oracle C Node::Init"
        c = O.csr_from_raw(row_id, seg, nbr, raw, T)
        row_ptr, type_end, prefix, type_prefix = c.row_ptr, c.type_end, c.prefix_w, c.type_prefix
    else:
        SUMS = "numpy cumsum per row"
        row_ptr = seg[::T].copy()
        type_end = (seg[1:].reshape(n, T) - row_ptr[:-1, None]).astype(np.int32)
        prefix = np.zeros(len(raw), np.float32)
        type_prefix = np.zeros((n, T), np.float32)
        for r in range(n):
            prefix[row_ptr[r]:row_ptr[r + 1]] = np.cumsum(raw[row_ptr[r]:row_ptr[r + 1]], dtype=np.float32)
            run = np.float32(0)
            for k in range(T):
                g = raw[seg[r * T + k]:seg[r * T + k + 1]]
                run = run + (np.cumsum(g, dtype=np.float32)[-1] if len(g) else np.float32(0))
                type_prefix[r, k] = run
    return euler_amd.Graph.from_csr(row_id, row_ptr, type_end, nbr, prefix, type_prefix, T)


def route_device(n, src, dst, typ, w):
    return euler_amd.Graph.from_edges(src, dst, edge_type=typ, weight=w, n_edge_types=T,
                                      nodes=torch.arange(1, n + 1, device="cuda"))


class UsedBytesPeak:
    """the largest (total - free) of the device while the block runs, polled every millisecond"""
    def __enter__(self):
        free, total = torch.cuda.mem_get_info()
        self.before = self.peak = total - free
        self.stop = False
        self.thread = threading.Thread(target=self.poll)
        self.thread.start()
        return self

    def poll(self):
        while not self.stop:
            free, total = torch.cuda.mem_get_info()
            self.peak = max(self.peak, total - free)
            time.sleep(0.001)

    def __exit__(self, *exc):
        self.stop = True
        self.thread.join()


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g = fn(*args)
    torch.cuda.synchronize()
    return g, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-edges", type=int, nargs="+", default=[24, 27])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    results = []
    for log2_e in a.log2_edges:
        n, src, dst, typ, w = make_edges(log2_e)
        e = src.numel()
        args = (n, src, dst, typ, w)
        # one run of each, not counted; their first row and hub row must be the same bytes (faster and
        # different is not faster)
        probe = np.array([1, n], np.uint64)
        g, _ = timed(route_device, *args)
        want = g.export_rows(probe)
        g.close()
        g, _ = timed(route_host, *args)
        got = g.export_rows(probe)
        g.close()
        rows = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, want))
        runs = {"host": [], "device": []}
        passes, peak_used, torch_rise, graph_bytes = {}, 0, 0, 0
        for _ in range(a.repeats):
            torch.cuda.reset_peak_memory_stats()
            held = torch.cuda.memory_allocated()
            with UsedBytesPeak() as used:
                g, dt = timed(route_device, *args)
            runs["device"].append(dt)
            passes = g.from_edges_pass_ms()
            peak_used = max(peak_used, used.peak - used.before)
            torch_rise = max(torch_rise, torch.cuda.max_memory_allocated() - held)
            graph_bytes = g.device_bytes
            g.close()
            g, dt = timed(route_host, *args)
            runs["host"].append(dt)
            g.close()
            print("# 2^%d edges: from_edges %.3f s, host route %.3f s" % (log2_e, runs["device"][-1], dt), flush=True)
        res = dict(log2_edges=log2_e, edges=e, nodes=n, edge_types=T, hub_entries=min(HUB, e // 4),
                   host_s=runs["host"], device_s=runs["device"], host_median_s=float(np.median(runs["host"])),
                   device_median_s=float(np.median(runs["device"])), device_pass_ms=passes,
                   device_peak_used_bytes_per_edge=peak_used / e, torch_allocator_rise_bytes_per_edge=torch_rise / e,
                   graph_bytes_per_edge=graph_bytes / e, rows_equal=rows, host_route_sums=SUMS)
        results.append(res)
        print(json.dumps(res), flush=True)
        del src, dst, typ, w
        torch.cuda.empty_cache()
    # the long rows' prefix pass alone: a graph that is only the hub row
    gen = torch.Generator(device="cuda").manual_seed(7)
    dst = torch.randint(1, 1000, (HUB,), device="cuda", generator=gen)
    src = torch.full((HUB,), 5000, device="cuda", dtype=torch.int64)
    typ = torch.randint(0, T, (HUB,), device="cuda", generator=gen, dtype=torch.int32)
    w = torch.rand(HUB, device="cuda", generator=gen) * 4 + 0.5
    hub_ms = []
    for _ in range(a.repeats + 1):
        g, _ = timed(lambda: euler_amd.Graph.from_edges(src, dst, edge_type=typ, weight=w, n_edge_types=T,
                                                        nodes=torch.tensor([5000], device="cuda")))
        hub_ms.append(g.from_edges_pass_ms()["prefix_long_rows"])
        g.close()
    res = dict(hub_row_entries=HUB, hub_prefix_ms=hub_ms[1:], hub_prefix_median_ms=float(np.median(hub_ms[1:])))
    results.append(res)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
