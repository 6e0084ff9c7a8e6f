#!/usr/bin/env python3
"""Benchmark of the sampling hot path on MI355X.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B]
                  [--nodes 100000000] [--edges 1000000000]
                  [--dump-outputs DIR] [--full]

Metric (BASELINE.json): sampled edges/sec, whole node, 2-hop fanout [25,10] on
a 100M-node / 1B-edge weighted power-law graph resident in HBM.  One "step" =
one minibatch of B roots through SampleFanout([25,10]) = B*275 sampled edges,
roots already in HBM.  With --gpus N > 1 (launched by torch.distributed.run,
one rank per GPU) the graph is hash-partitioned over the ranks (owner(id) =
id % N) and every hop does the id / result all-to-all over RCCL; every rank
samples its own B roots per step (weak scaling).

Rank 0 prints ONE JSON line: metric/value/unit/ms_per_step/...  A plain run sets
up, warms up, times the K steps ONCE and prints the line.  With --full it also
reports (every --no-* option below switches one of them off again):
  repeats       the K-step loop timed --repeats times (default 5), the median kept
  roofline      the step's launch timed with HIP events on its own stream;
                achieved = algorithmic bytes / time
  cpu_baseline  the reference sampler (oracle/_ref: reference sources + RNG
                seam) timed on the host cores on a bounded sample of the same
                workload family
  and the oracle parity check of the last step, the one-stream and sustained
  loops, the B = 1 024 latency leg, the secondary legs, the replicated-graph leg
  of a sharded run.  --workload hetero / deepwalk run their whole legs either way.
--dump-outputs DIR writes a fixed, seeded sample of the last timed step's
outputs (ids and types as float64, weights as float32) to DIR/<name>.npy.
"""
import argparse
import gc
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the legs live in bench_legs/ (one module per workload family); their names stay importable from here
from bench_legs import common as _common                                  # noqa: E402
from bench_legs.common import *                                           # noqa: E402,F401,F403
from bench_legs.cpu import *                                              # noqa: E402,F401,F403
from bench_legs.latency import *                                          # noqa: E402,F401,F403
from bench_legs.hetero import *                                           # noqa: E402,F401,F403
from bench_legs.deepwalk import *                                         # noqa: E402,F401,F403
from bench_legs.fanout_legs import *                                      # noqa: E402,F401,F403
from bench_legs.sage import *                                             # noqa: E402,F401,F403
from bench_legs.nodes import *                                            # noqa: E402,F401,F403
from bench_legs.host_boundary import run_host_boundary_leg                # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=131072,
                    help="roots per step per GPU")
    ap.add_argument("--nodes", type=int, default=100_000_000)
    ap.add_argument("--edges", type=int, default=1_000_000_000)
    ap.add_argument("--cpu-nodes", type=int, default=20_000_000,
                    help="graph size of the CPU baseline (SURVEY 8(d): 20M nodes / 200M "
                         "edges; reduced automatically when the host's RAM does not hold it)")
    ap.add_argument("--cpu-protocol", choices=["quick", "full"], default="quick",
                    help="full = 5 warm-up + 30 timed rounds for every cell (minutes)")
    ap.add_argument("--streams", type=int, default=3,
                    help="unsharded path: consecutive minibatches alternate between this many "
                         "HIP streams (each with its own scratch): the latency-bound phases of "
                         "one minibatch (first hop, duplicate detection, sampling of the "
                         "distinct roots) overlap the bandwidth-bound expansion of the other - "
                         "the reference likewise keeps 8 queries in flight "
                         "(client/query_proxy.cc:205-210).  Same box, 20 steps x 5: 1 stream 0.229 ms per "
                         "step, 2: 0.212-0.223, 3: 0.206 (and the steadiest), 4: 0.225")
    ap.add_argument("--workload", choices=["metric", "products", "hetero", "deepwalk"],
                    default="metric",
                    help="metric = BASELINE.json's headline (configs[2]); products = configs[1] "
                         "(ogbn-products-shaped CSR, uniform SampleNeighbor fanout [25,10]); "
                         "hetero = configs[4] on one GPU (8 edge types: typed sampling k = 1 / "
                         "3 of 8 / all + 128-d feature gather + scatter_mean); deepwalk = "
                         "configs[3] on one GPU (random_walk length 40)")
    ap.add_argument("--tuning", default="",
                    help="A/B only: comma-separated key=value pairs for euler_gpu_set_tuning")
    ap.add_argument("--repeats", type=int, default=None,
                    help="the K-step timed loop is repeated this many times; the line "
                         "reports the median repetition (and lists all); default 5 with "
                         "--full, else 1")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: repeats, parity check, roofline, one-stream / "
                         "sustained loops, latency, secondary and replicated-graph legs, "
                         "cpu_baseline (a plain run times the K steps once and stops)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write a seeded sample of the last step's "
                         "outputs as DIR/<name>.npy (float32 / float64, < 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--n2v", action="store_true", help="deepwalk workload: also time node2vec")
    ap.add_argument("--unfused-aggregation", action="store_true",
                    help="hetero workload: gather, then scatter_mean (two passes over the E x D block)")
    ap.add_argument("--hetero-separate", action="store_true",
                    help="hetero workload: one sample_neighbor + one aggregation op per edge-type set "
                         "(round 3's step) instead of the one-enqueue form")
    ap.add_argument("--check-roots", type=int, default=4096,
                    help="roots of the last timed step compared with the CPU oracle after the timed region")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--sustain-steps", type=int, default=4000,
                    help="metric workload, one GPU: after the K timed steps, this many more steps "
                         "(>= 1 s of device time) are timed as ONE region and reported as "
                         "config.sustained - the K-step median is a ~5 ms burst (0 = skip)")
    ap.add_argument("--large-batch", type=int, default=1048576,
                    help="roots of the second roofline launch (SURVEY 8(d) config 3: B >= 1M per "
                         "launch for the HBM-roofline run; 0 = skip)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the short products / hetero / deepwalk (+ node2vec) legs the default "
                         "single-GPU metric run appends under config.secondary")
    ap.add_argument("--no-small-batch", action="store_true",
                    help="skip the B = 1 024 latency leg (profiling runs: its 1 000 small "
                         "launches would share kernel names with the step's)")
    ap.add_argument("--pipeline", type=int, default=4,
                    help="sharded path: minibatches in flight, interleaved hop by hop "
                         "from one host thread (each on its own sampler and HIP "
                         "stream): while the host waits for one batch's bucket sizes "
                         "the GPU runs the others' kernels and exchanges (one rank, round 6: "
                         "0.39-0.40 ms / step with 1, 0.338 with 2, 0.321 with 3, 0.309 with 4, "
                         "0.323 with 6 or 8)")
    ap.add_argument("--oversubscribe", action="store_true",
                    help="functional check only: when fewer GPUs are visible than --gpus, "
                         "let the ranks share them (rank r on GPU r %% visible) with a "
                         "gloo host-staged transport (RCCL refuses two ranks per device); "
                         "the line then says so and is not a scaling number")
    ap.add_argument("--replicas", action="store_true",
                    help="--gpus N: every rank holds the WHOLE graph (68.6 GB of 288) and runs the "
                         "unsharded step on its own roots - no exchange (SURVEY H7); the default "
                         "--gpus N run is hash-sharded and reports this mode beside it "
                         "(config.replicas)")
    ap.add_argument("--no-replicas-leg", action="store_true",
                    help="--gpus N: skip the replicated-graph leg of the sharded run")
    ap.add_argument("--force-sharded", action="store_true",
                    help="run the multi-GPU sampler (unique / split / all-to-all / "
                         "merge / gather) even on one rank: measures its overhead")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 5 if args.full else 1
    return args


_DEFERRED = None        # a list while a process group is up: the line is printed after its teardown


def secondary_legs(args, G, p_g):
    """BASELINE configs[1], [3], [4] as short legs of the default run (rank 0, one GPU), each
    with a spot check against the oracle at bench scale: {value, ms_per_step, roofline_frac,
    parity_checked}."""
    import copy
    sec = {}
    t0 = time.time()
    try:
        a = copy.copy(args)
        a.steps, a.warmup, a.repeats, a.n2v = 3, 1, 3, True
        d = run_deepwalk(a, G, p_g, quiet=True)
        sec["deepwalk"] = {"value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"],
                           "roofline_frac": d["roofline"]["frac"],
                           "parity_checked": d["config"]["parity_checked_steps"],
                           "workload": d["config"]["workload"]}
        n2 = d["config"]["node2vec"]
        sec["node2vec"] = {"value": n2["steps_per_s"], "unit": "walker steps/s", "ms_per_step": n2["ms"],
                           "roofline_frac": n2["frac"], "parity_checked": n2["parity_checked_steps"],
                           "workload": "p = 0.25, q = 4: %d walkers x %d steps on the metric graph"
                                       % (n2["walkers"], n2["walk_len"])}
    except Exception as e:          # a side measurement must not fail the bench
        sec["deepwalk"] = {"error": repr(e)}
    for name_, fn_ in (("fanout_unique_rows", run_unique_leg), ("sage_blocks", run_sage_leg)):
        try:
            sec[name_] = fn_(args, G, p_g)
        except Exception as e:
            sec[name_] = {"error": repr(e)}
    try:
        sec.update(run_node_legs(args, G, p_g))
    except Exception as e:
        sec["sample_node"] = {"error": repr(e)}
    try:
        sec["host_boundary"] = run_host_boundary_leg(args, G, p_g)
    except Exception as e:
        sec["host_boundary"] = {"error": repr(e)}
    try:
        sec["products"] = run_products_leg(args)
    except Exception as e:
        sec["products"] = {"error": repr(e)}
    try:
        sec["metric_hashed_T2"] = run_hashed_leg(args)
    except Exception as e:
        sec["metric_hashed_T2"] = {"error": repr(e)}
    try:      # ... with all weights 1.0: the shape of every dataset the reference ships
        sec["metric_hashed_T2_unweighted"] = run_hashed_leg(args, weighted=False)
    except Exception as e:
        sec["metric_hashed_T2_unweighted"] = {"error": repr(e)}
    try:
        a = copy.copy(args)
        a.steps, a.warmup, a.repeats = 10, 3, 3
        h = run_hetero(a, quiet=True)
        sec["hetero"] = {"value": h["value"], "unit": h["unit"], "ms_per_step": h["ms_per_step"],
                         "roofline_frac": h["roofline"]["frac"],
                         "parity_checked": h["config"]["parity_checked_edges"],
                         "workload": h["config"]["workload"]}
    except Exception as e:
        sec["hetero"] = {"error": repr(e)}
    sec["seconds"] = round(time.time() - t0, 1)
    return sec


DUMP_ROOTS = 4096       # --dump-outputs: roots of the last step whose rows are written


def dump_outputs(dirname, roots, out):
    """The last timed step as its caller receives it - (neighbors [roots, hop 1, hop 2], weights,
    types) of sample_fanout - restricted to DUMP_ROOTS roots drawn with a fixed seed (the whole
    step is ~0.5 GB): DIR/<name>.npy, ids and types as float64 (exact below 2^53), weights float32."""
    nbrs, wts, tps = out
    B = roots.numel()
    sel = np.sort(np.random.default_rng(0).choice(B, min(B, DUMP_ROOTS), replace=False))
    sel_t = torch.as_tensor(sel, device=roots.device)
    arrays = {"sample_root_index": sel.astype(np.float64),
              "roots": roots[sel_t].cpu().numpy().astype(np.float64)}
    for h in range(len(wts)):
        def rows(x, dt):
            return x.reshape(B, -1)[sel_t].cpu().numpy().astype(dt)
        arrays["hop%d_ids" % (h + 1)] = rows(nbrs[h + 1], np.float64)
        arrays["hop%d_weights" % (h + 1)] = rows(wts[h], np.float32)
        arrays["hop%d_types" % (h + 1)] = rows(tps[h], np.float64)
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def launch_ranks(args):
    """`python bench.py --gpus N` with no launcher around it: start the N ranks
    ourselves (torch.distributed.run, one process per GPU, rendezvous on
    127.0.0.1) and pass their output through.  Returns the exit code."""
    import socket
    import subprocess
    visible = torch.cuda.device_count()
    if visible < args.gpus and not args.oversubscribe:
        print("bench.py: --gpus %d but only %d GPU(s) visible (use --oversubscribe for a "
              "functional check on fewer devices)" % (args.gpus, visible), file=sys.stderr)
        return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and world > 1:
        args.gpus = world
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    visible = torch.cuda.device_count()
    shared_gpus = world > visible           # ranks share devices: functional check only
    if shared_gpus and not args.oversubscribe:
        raise SystemExit("bench.py: %d ranks but %d GPU(s) visible (pass --oversubscribe)"
                         % (world, visible))
    local_rank %= visible
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    replicas = bool(args.replicas) and world > 1
    sharded = (world > 1 and not replicas) or args.force_sharded
    backend = "gloo" if shared_gpus else "nccl"
    if sharded or world > 1:
        _common._defer_lines()
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29512")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    import euler_amd
    from euler_amd import _lib
    L = _lib.lib()
    for kv in filter(None, args.tuning.split(",")):
        k_, v_ = kv.split("=")
        _lib.check(L.euler_gpu_set_tuning(int(k_), int(v_)))
    if args.workload in ("hetero", "deepwalk"):
        if args.dump_outputs:
            raise SystemExit("bench.py: --dump-outputs covers the metric / products workloads")
        (run_hetero if args.workload == "hetero" else run_deepwalk)(args)
        _teardown(sharded or world > 1)
        return
    weighted = args.workload != "products"
    if args.workload == "products":
        # configs[1]: ogbn-products' public shape (2 449 029 nodes, 61 859 140 undirected =
        # 123 718 280 directed edges), all weights 1.0; `ogb` is not installed and there is
        # no network: a degree-sequence-matched synthetic graph of that size
        args.nodes, args.edges = 2_449_029, 123_718_280
        args.no_cpu_baseline = True

    t0 = time.time()
    p = euler_amd.synth_params(GRAPH_SEED, args.nodes, args.edges, weighted=weighted)
    g_parts = 1 if replicas else world
    G = euler_amd.Graph.synthetic(p, device=local_rank, partitions=g_parts,
                                  shard_index=0 if replicas else rank, shards=g_parts)
    G.set_seed(GRAPH_SEED)
    torch.cuda.synchronize()
    build_s = time.time() - t0

    B = args.batch
    n_steps = args.steps + args.warmup
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + rank)
    roots = torch.randint(1, args.nodes + 1, (n_steps, B), generator=gen,
                          device=dev, dtype=torch.int64)
    et = [[0], [0]]
    default_node = args.nodes + 1

    def sync():
        if sharded or world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    sustained = None
    if sharded:
        # A sharded hop makes the host wait once (the bucket sizes of its front
        # end).  K minibatches are kept in flight from ONE host thread
        # (euler_amd.distributed.run_interleaved): each has its own sampler
        # (front-end handle, id-indexed table, counts mailbox) and HIP stream, the
        # hops of the batches alternate, and every rank issues the same sequence
        # of collectives because the schedule does not depend on the data.
        from euler_amd.distributed import gpu_sharded_sampler, run_interleaved
        K = max(1, min(args.pipeline, args.steps))
        samplers = [gpu_sharded_sampler(G, partitions=world) for _ in range(K)]
        streams = [torch.cuda.Stream(device=dev) for _ in range(K)]

        trace = [] if os.environ.get("EULER_BENCH_TRACE") else None

        def run(first, last):
            def make(j):
                if trace is not None:
                    trace.append((first + j, time.perf_counter(),
                                  torch.cuda.memory_stats()["num_device_alloc"]))
                return samplers[j % K].sample_fanout_steps(
                    roots[first + j], et, FANOUT, default_node, call_id=2 * (first + j))
            kept = [None]                    # only the last minibatch's outputs stay alive

            def consume(job, value):
                if job == last - first - 1:
                    kept[0] = value
            run_interleaved(make, last - first, K,
                            enter=lambda k: torch.cuda.stream(streams[k]), on_result=consume)
            res = kept
            for st_ in streams:
                st_.synchronize()
            return res[-1] if res else None

        torch.cuda.synchronize()          # roots were produced on the default stream
        # The distinct-id counts differ from batch to batch, so the caching allocator
        # keeps meeting new tensor sizes for a while (130 device allocations over the
        # first 20 steps, none afterwards): PREWARM extra untimed steps on top of the W
        # the caller asked for keep those out of the timed region.
        for _ in range(PREWARM // max(n_steps, 1) + 1):
            run(0, min(n_steps, PREWARM))
        run(0, args.warmup)
        sync()
        gc.collect(); gc.freeze(); gc.disable()      # a gen-2 collection costs ~40 ms
        wire0 = sum(s_.bytes_sent for s_ in samplers)
        rep_secs = []
        for _rep in range(max(1, args.repeats)):
            sync()
            t0 = time.perf_counter()
            out = run(args.warmup, n_steps)
            sync()
            rep_secs.append(time.perf_counter() - t0)
        gc.enable()
        wire_bytes = (sum(s_.bytes_sent for s_ in samplers) - wire0) / len(rep_secs)
        if trace is not None and rank == 0:
            tail = trace[-(n_steps - args.warmup):]
            print("trace (step, ms since previous job started, device allocs so far):",
                  [(a[0], round((a[1] - b[1]) * 1e3, 2), a[2]) for a, b in zip(tail[1:], tail[:-1])],
                  file=sys.stderr)
    def unsharded_run(Gx, extras=True, settle=False):
        """The K steps on the unsharded graph Gx (this rank's whole graph): --streams callers'
        streams alternating; returns (rep_secs, one_stream secs, last outputs, sustained)."""
        def step(i):
            return Gx.sample_fanout(roots[i % n_steps], et, FANOUT, default_node, call_id=2 * (i % n_steps))

        n_streams = max(1, args.streams)
        side = [torch.cuda.Stream(device=dev) for _ in range(n_streams)] if n_streams > 1 else None

        def loop(first, last, streams):
            res = None
            if streams is None:
                for i in range(first, last):
                    res = step(i)
            else:
                for i in range(first, last):
                    with torch.cuda.stream(streams[i % len(streams)]):
                        res = step(i)
            return res

        torch.cuda.synchronize()              # roots were produced on the default stream
        out_ = loop(0, max(args.warmup, 2 * n_streams), side)
        sync()
        gc.collect(); gc.freeze(); gc.disable()      # a gen-2 collection costs ~40 ms
        one_stream_ = []
        # the same K steps on ONE stream, for the record (settle: run, not reported - a plain run
        # then times the same state of the device as --full: 0.225 ms per step without, 0.199-0.210 with)
        if side is not None and (extras or settle):
            loop(0, args.warmup, None)
            for _rep in range(3):
                sync()
                t0 = time.perf_counter()
                loop(args.warmup, n_steps, None)
                sync()
                one_stream_.append(time.perf_counter() - t0)
            loop(0, 2 * n_streams, side)
            if not extras:
                one_stream_ = []
        rep_secs_ = []
        for _rep in range(max(1, args.repeats)):
            sync()
            t0 = time.perf_counter()
            out_ = loop(args.warmup, n_steps, side)
            sync()
            rep_secs_.append(time.perf_counter() - t0)
        # the same loop as ONE long region (>= 1 s of device time): what the K-step bursts above
        # are extrapolated to (roots cycle through the n_steps batches; call ids keep counting)
        sustained_ = None
        if world == 1 and extras and args.sustain_steps > 0 and side is not None:
            ns_ = args.sustain_steps
            sync()
            t0 = time.perf_counter()
            for i in range(ns_):
                with torch.cuda.stream(side[i % n_streams]):
                    Gx.sample_fanout(roots[i % n_steps], et, FANOUT, default_node, call_id=2 * (n_steps + i))
            sync()
            dt_ = time.perf_counter() - t0
            sustained_ = {"steps": ns_, "seconds": round(dt_, 4), "ms_per_step": round(dt_ / ns_ * 1e3, 4),
                          "edges_per_s": B * (FANOUT[0] + FANOUT[0] * FANOUT[1]) * ns_ / dt_,
                          "streams": n_streams}
        gc.enable()
        return rep_secs_, one_stream_, out_, sustained_

    def reduce_secs(secs):
        if world <= 1:
            return secs
        t = torch.tensor(secs, device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)          # slowest rank, per repetition
        return [float(x) for x in t.tolist()]

    replicas_leg = None
    one_stream = []
    if not sharded:
        rep_secs, one_stream, out, sustained = unsharded_run(G, extras=args.full, settle=True)
    elif world > 1 and args.full and not args.no_replicas_leg and args.workload == "metric":
        # beside the hash-sharded headline: every rank with the WHOLE graph in its own HBM
        # (68.6 GB of 288), the unsharded step on its own roots - what sharding costs
        try:
            Gr = euler_amd.Graph.synthetic(p, device=local_rank)
            Gr.set_seed(GRAPH_SEED)
            r_secs, _one, _out, _sus = unsharded_run(Gr, extras=False)
            r_secs = reduce_secs(r_secs)
            r_el = float(np.median(r_secs))
            replicas_leg = {"value": B * 275 * world * args.steps / r_el, "unit": "sampled edges/s",
                            "ms_per_step": r_el / args.steps * 1e3, "graph_bytes_per_gpu": Gr.device_bytes,
                            "repeat_ms_per_step": [round(x / args.steps * 1e3, 4) for x in r_secs],
                            "what": "graph replicated on every GPU, no exchange (SURVEY H7): the same "
                                    "roots, steps and timing protocol as the sharded headline"}
            del Gr, _out
            torch.cuda.empty_cache()
        except Exception as e:
            replicas_leg = {"error": repr(e)}
    exchanged = None
    wire_dev = dev if backend == "nccl" else "cpu"
    rep_secs = reduce_secs(rep_secs)
    # EXACTLY K steps were timed, `repeats` times over; the line reports the median
    elapsed = float(np.median(rep_secs))
    if world > 1 and sharded:
        t = torch.tensor([float(wire_bytes)], device=wire_dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        exchanged = float(t.item()) / args.steps          # bytes / step, all ranks
    elif sharded:
        exchanged = 0.0                                   # one rank: self exchanges only
    edges_per_step = B * (FANOUT[0] + FANOUT[0] * FANOUT[1]) * world
    value = edges_per_step * args.steps / elapsed

    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, roots[n_steps - 1], out)

    # ---- parity check at full size, after the timed region: --check-roots roots of the last step
    # (default 4 096 = 1.1 M sampled edges) against the CPU oracle fed with rows exported from HBM
    # (oracle/step_check.py: all of their hop-1 samples, every hop-2 position against the first
    # position of its node, one row per distinct hop-1 child against the oracle); single GPU only
    checked = None
    if (world == 1 or replicas) and rank == 0 and args.full and not args.no_check:
        from oracle import oracle as O
        from oracle.step_check import check_fanout_step
        last = n_steps - 1
        n_chk = max(1, min(B, args.check_roots))
        sel = torch.as_tensor(np.sort(np.random.default_rng(0).choice(B, n_chk, replace=False))).to(dev)
        r_sel = roots[last][sel]
        c1_, c2_ = FANOUT
        sub_n = [r_sel, out[0][1].reshape(B, c1_)[sel].reshape(-1), out[0][2].reshape(B, c1_ * c2_)[sel].reshape(-1)]
        sub_w = [out[1][0].reshape(B, c1_)[sel].reshape(-1), out[1][1].reshape(B, c1_ * c2_)[sel].reshape(-1)]
        sub_t = [out[2][0].reshape(B, c1_)[sel].reshape(-1), out[2][1].reshape(B, c1_ * c2_)[sel].reshape(-1)]
        # the rows in HBM are the rows the HOST generator (oracle/eo_synth.c) produces for
        # these ids - a generator fault at full size cannot hide behind "oracle fed with
        # exported rows"
        need = np.unique(np.concatenate([r_sel.cpu().numpy()[:64], sub_n[1].cpu().numpy()[:1600]])).astype(np.uint64)
        need = need[need <= args.nodes]
        rp, te, nb, pw, tp = G.export_rows(need)
        po = O.SynthParams()
        for f_, _t in po._fields_:
            setattr(po, f_, getattr(p, f_))
        for j_ in np.random.default_rng(1).choice(len(need), min(256, len(need)), replace=False):
            h_ = O.synth_csr(po, int(need[j_]) - 1, int(need[j_]))
            b_, e_ = int(rp[j_]), int(rp[j_ + 1])
            assert np.array_equal(h_.nbr, nb[b_:e_]) and np.array_equal(h_.prefix_w, pw[b_:e_]), \
                "device generator differs from the host generator at node %d" % int(need[j_])
        checked, _distinct = check_fanout_step(G, O.OracleGraph, O.CSR, GRAPH_SEED, 2 * last, r_sel, sub_n, sub_w,
                                               sub_t, FANOUT, default_node, args.nodes)
        del sub_n, sub_w, sub_t

    # ---- roofline leg: the launches of a step, phase by phase, HIP events on
    # the stream the kernels run on.  Hop 1 samples the caller's roots directly;
    # hop 2 counts duplicate roots on device and (when they repeat) samples the
    # distinct ones once and expands.  The dominant kernel is K1
    # (SampleNeighborPivotKernel): its algorithmic bytes are SURVEY 8(d)'s
    # per-root / per-edge figure summed over the roots it actually processes.
    roofline = None
    fused = not sharded and "27=0" not in args.tuning.split(",")
    if not sharded and not fused:
        raise SystemExit("bench.py: --tuning 27=0 (hop-by-hop fanout) has no roofline leg any more; "
                         "use tools/ab_key.py for that A/B")
    if rank == 0 and fused and args.full:
        # The step is ONE kernel (fanout_local.h: hop 1, the duplicate children found inside
        # the wave, hop 2 once per distinct child, the rows streamed out): the roofline object
        # is that launch.  Algorithmic bytes = SURVEY 8(d), evaluated on the roots the step
        # really has: K1 over the batch (hop 1) + K1 over the DISTINCT hop-2 roots (counted
        # globally, as the reference's ID_UNIQUE would - the kernel itself samples ~1.3x as
        # many, duplicates across waves) + 8 + 4 per hop-2 input id (dedup) + 16 per
        # expanded output edge (gather).
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        et1 = (C.c_int32 * 1)(0)
        layers = len(FANOUT)
        cnt_a = (C.c_int32 * layers)(*FANOUT)
        et_a = (C.c_int32 * layers)(*([0] * layers))
        r = roots[n_steps - 1].contiguous()
        o_n, o_w, o_t, m = [], [], [], r.numel()
        for c in FANOUT:
            m *= c
            o_n.append(torch.empty(m, dtype=torch.int64, device=dev))
            o_w.append(torch.empty(m, dtype=torch.float32, device=dev))
            o_t.append(torch.empty(m, dtype=torch.int32, device=dev))
        wsz = int(L.euler_gpu_sample_fanout_workspace(r.numel(), cnt_a, layers))
        fws = torch.empty(max(wsz, 16), dtype=torch.uint8, device=dev)
        pn = (C.c_void_p * layers)(*[t.data_ptr() for t in o_n])
        pw_ = (C.c_void_p * layers)(*[t.data_ptr() for t in o_w])
        pt = (C.c_void_p * layers)(*[t.data_ptr() for t in o_t])
        torch.cuda.synchronize()
        ms = C.c_float(0)
        _lib.check(L.euler_gpu_time_sample_fanout(
            G._h, st, GRAPH_SEED, C.c_void_p(r.data_ptr()), r.numel(), et_a, 1, cnt_a, layers,
            default_node, pn, pw_, pt, C.c_void_p(fws.data_ptr()), 20, C.byref(ms)))

        kernel_name = (L.euler_gpu_last_fanout_kernel() or b"").decode() or "SampleFanoutLeanKernel"

        def algo_bytes(x, cnt):
            b = C.c_double(0)
            _lib.check(L.euler_gpu_sample_neighbor_algo_bytes(
                G._h, st, C.c_void_p(x.data_ptr()), x.numel(), et1, 1, cnt, C.byref(b)))
            return b.value
        hop2_roots = o_n[0]
        uniq2 = torch.unique(hop2_roots).contiguous()
        b1 = algo_bytes(r, FANOUT[0])
        b2 = algo_bytes(uniq2, FANOUT[1])
        n2 = hop2_roots.numel()
        b_dedup = 12.0 * n2
        b_gather = 16.0 * n2 * FANOUT[1]
        total_b = b1 + b2 + b_dedup + b_gather
        achieved = total_b / (ms.value * 1e-3) / 1e9
        traffic = None
        pmc = os.path.join(ROOT, "profiles", "pmc_latest.json")
        pmc_rec = {}
        if os.path.exists(pmc):
            try:
                pmc_rec = json.load(open(pmc))
                if pmc_rec.get("batch") == B and pmc_rec.get("nodes") == args.nodes and \
                        pmc_rec.get("kernel") == kernel_name:
                    traffic = pmc_rec.get("hbm_bytes_per_launch")
                else:
                    pmc_rec = {}
            except Exception:
                traffic = None
                pmc_rec = {}
        one_ms = (float(np.median(one_stream)) / args.steps * 1e3) if one_stream else None
        rd_req = pmc_rec.get("read_requests_per_launch")
        roofline = {
            "kernel": kernel_name, "bound": "hbm",
            "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
            "traffic_note": "profiles/pmc_latest.json: TCC_EA0_RDREQ x 128 B + TCC_EA0_WRREQ x 64 B per "
                            "launch (separate rocprofv3 --pmc pass; a read request moves a 128-byte line, "
                            "FETCH_SIZE tallies it at 64 B - calibration in profiles/r2_pmc_summary.json)",
            "algorithmic_bytes_per_launch": round(total_b, 1),
            "avg_launch_ms": round(ms.value, 4),
            # what the three-stream headline must not be mistaken for: the same
            # bytes over ONE caller's step time (enqueue gaps included), and over the headline's
            "one_stream_frac": (round(total_b / (one_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if one_ms else None),
            "headline_streams_frac": round(total_b / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS, 5),
            # 128-byte lines the launch reads from the fabric (TCC_EA0_RDREQ of the same --pmc pass as
            # `traffic`) per second of the launch: the chip completes ~48 G random lines/s when every
            # line is ONE request and 19.5 G when a lane makes four requests for its line, as a
            # draw here does (tools/ubench_block.hip, profiles/r6_ubench_block.txt)
            "read_lines_per_s": (round(rd_req / (ms.value * 1e-3), 1) if rd_req else None),
            "launches_per_step": [{
                "roots": int(r.numel()), "fanout": FANOUT, "hop2_roots": int(n2),
                "hop2_distinct_roots": int(uniq2.numel()),
                "k1_hop1_algorithmic_bytes": b1, "k1_hop2_distinct_algorithmic_bytes": b2,
                "dedup_algorithmic_bytes": b_dedup, "gather_algorithmic_bytes": b_gather}],
            "note": "the whole step is this one launch, timed alone on one stream with HIP events "
                    "(euler_gpu_time_sample_fanout, 20 calls); bytes = SURVEY 8(d) summed over the "
                    "step: K1 of hop 1 over the batch, K1 of hop 2 over the globally distinct hop-2 "
                    "roots, 8 + 4 per hop-2 input id, 16 per expanded output edge",
        }
        if args.large_batch > 0 and args.large_batch != B:
            # "B >= 1M per launch for the HBM-roofline run": the same launch
            # over 1 048 576 roots (8 rounds of the chip instead of 6.4: the tail and the launch
            # are a smaller share), bytes counted the same way
            try:
                BL = args.large_batch
                gl = torch.Generator(device=dev); gl.manual_seed(555)
                rl = torch.randint(1, args.nodes + 1, (BL,), generator=gl, device=dev, dtype=torch.int64)
                ol_n, ol_w, ol_t, m = [], [], [], BL
                for c in FANOUT:
                    m *= c
                    ol_n.append(torch.empty(m, dtype=torch.int64, device=dev))
                    ol_w.append(torch.empty(m, dtype=torch.float32, device=dev))
                    ol_t.append(torch.empty(m, dtype=torch.int32, device=dev))
                wl = torch.empty(max(int(L.euler_gpu_sample_fanout_workspace(BL, cnt_a, layers)), 16),
                                 dtype=torch.uint8, device=dev)
                pln = (C.c_void_p * layers)(*[t.data_ptr() for t in ol_n])
                plw = (C.c_void_p * layers)(*[t.data_ptr() for t in ol_w])
                plt_ = (C.c_void_p * layers)(*[t.data_ptr() for t in ol_t])
                msl = C.c_float(0)
                torch.cuda.synchronize()
                _lib.check(L.euler_gpu_time_sample_fanout(
                    G._h, st, GRAPH_SEED, C.c_void_p(rl.data_ptr()), BL, et_a, 1, cnt_a, layers,
                    default_node, pln, plw, plt_, C.c_void_p(wl.data_ptr()), 5, C.byref(msl)))
                u2 = torch.unique(ol_n[0]).contiguous()
                nl2 = ol_n[0].numel()
                tb = algo_bytes(rl, FANOUT[0]) + algo_bytes(u2, FANOUT[1]) + 12.0 * nl2 + 16.0 * nl2 * FANOUT[1]
                # the same 64-root oracle check on this launch's output
                chk = None
                if not args.no_check:
                    sel = np.random.default_rng(3).choice(BL, 64, replace=False)
                    st_t = torch.as_tensor(sel).to(dev)
                    r0 = rl[st_t].cpu().numpy()
                    h1 = ol_n[0].reshape(BL, FANOUT[0])[st_t].cpu().numpy()
                    h2 = ol_n[1].reshape(BL, -1)[st_t].cpu().numpy()
                    need_l = np.concatenate([r0, h1.reshape(-1)])
                    OGl = _oracle_rows(G, p, need_l[(need_l >= 1) & (need_l <= args.nodes)], 1)
                    # euler_gpu_time_sample_fanout draws iteration it with call ids it * layers + h
                    onl, _, _ = OGl.sample_fanout(GRAPH_SEED, 4 * layers, r0, et, FANOUT, default_node)
                    assert np.array_equal(onl[0], h1.reshape(-1)) and np.array_equal(onl[1], h2.reshape(-1)), \
                        "B = 1M launch: sampled ids differ from the oracle"
                    chk = int(64 * 275)
                roofline["large_batch"] = {
                    "roots": BL, "avg_launch_ms": round(msl.value, 4),
                    "algorithmic_bytes_per_launch": round(tb, 1),
                    "achieved": round(tb / (msl.value * 1e-3) / 1e9, 2), "unit": "GB/s",
                    "frac": round(tb / (msl.value * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                    "edges_per_s": BL * 275 / (msl.value * 1e-3),
                    "hop2_distinct_roots": int(u2.numel()), "parity_checked_edges": chk}
                del ol_n, ol_w, ol_t, wl, rl, u2
                torch.cuda.empty_cache()
            except Exception as e:          # a side measurement must not fail the bench
                roofline["large_batch"] = {"error": repr(e)}
    if not fused and args.full:
        # The sharded step's own launches (every rank): the owners' pass of a hop is
        # euler_gpu_sample_neighbor_packed over the DISTINCT ids a rank is asked for - K1
        # (SampleNeighborPivotKernel, one sample per lane, wire rows written directly).  Timed
        # alone with HIP events on its stream, over the ids this rank's own batch asks for
        # mapped onto ids this rank owns (a rank is asked for as many as it asks, in expectation):
        # hop 1 = the distinct roots, hop 2 = the distinct hop-1 samples.  Bytes = SURVEY 8(d)'s
        # K1 formula over exactly those ids.
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        et1 = (C.c_int32 * 1)(0)

        def own(x):
            if world > 1 and sharded:      # a shard owns ids == rank (mod world)
                x = (x // world) * world + (rank if rank else world)
                x = torch.clamp(x, max=args.nodes - world)
            return torch.unique(x).contiguous()

        def algo_bytes(x, cnt):
            b = C.c_double(0)
            _lib.check(L.euler_gpu_sample_neighbor_algo_bytes(
                G._h, st, C.c_void_p(x.data_ptr()), x.numel(), et1, 1, cnt, C.byref(b)))
            return b.value
        hop_ids = [own(roots[n_steps - 1]), own(out[0][1].reshape(-1))]
        k1_ms, k1_bytes, phases = [], [], []
        for h, x in enumerate(hop_ids):
            cnt = FANOUT[h]
            ms_h = _events(lambda: G.sample_neighbor_packed(x, [0], cnt, default_node, call_id=h), 10)
            kb = algo_bytes(x, cnt)
            k1_ms.append(ms_h); k1_bytes.append(kb)
            phases.append({"hop": h, "distinct_ids_sampled": int(x.numel()), "count": cnt,
                           "k1_ms": round(ms_h, 4), "k1_algorithmic_bytes": kb,
                           "frac": round(kb / (ms_h * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})
        # the requester's side of hop 2, for the record: expansion of the answers to positions
        try:
            from euler_amd import ops as _ops
            n2 = out[0][1].numel()
            rows2 = G.sample_neighbor_packed(hop_ids[1], [0], FANOUT[1], default_node, call_id=1)
            pos2 = torch.randint(0, hop_ids[1].numel(), (n2,), device=dev, dtype=torch.int32)
            ms_x = _events(lambda: _ops.expand_packed(pos2, rows2, FANOUT[1], 0), 10)
            xb = 16.0 * n2 * FANOUT[1] + 4.0 * n2 + rows2.numel() * 4.0
            phases.append({"hop": 1, "expand_ms": round(ms_x, 4), "expand_algorithmic_bytes": xb,
                           "expand_GBps": round(xb / (ms_x * 1e-3) / 1e9, 1)})
            del rows2, pos2
        except Exception as e:
            phases.append({"expand_error": repr(e)})
        achieved = sum(k1_bytes) / (sum(k1_ms) * 1e-3) / 1e9
        per_rank = None
        if world > 1:
            t = torch.tensor([sum(k1_bytes), sum(k1_ms)], device=wire_dev, dtype=torch.float64)
            allt = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(allt, t)
            per_rank = [{"rank": r_, "frac": round(float(x_[0]) / (float(x_[1]) * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                         "k1_ms": round(float(x_[1]), 4)} for r_, x_ in enumerate(allt)]
            achieved = float(np.mean([x_["frac"] for x_ in per_rank])) * HBM_PEAK_GBS
        traffic = None
        pmc = os.path.join(ROOT, "profiles", "pmc_sharded_latest.json")
        if os.path.exists(pmc):
            try:
                rec = json.load(open(pmc))
                if rec.get("batch") == B and rec.get("nodes") == args.nodes and \
                        "SampleNeighborPivotKernel" in rec.get("kernel", ""):
                    traffic = rec.get("hbm_bytes_per_launch")
            except Exception:
                traffic = None
        if rank == 0:
            roofline = {
                "kernel": "SampleNeighborPivotKernel (owners' pass of a sharded hop, packed wire rows)",
                "bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
                "traffic": traffic,
                "traffic_note": "profiles/pmc_sharded_latest.json: TCC_EA0_RDREQ x 128 B + WRITE_SIZE per "
                                "launch of this kernel in the sharded step (separate rocprofv3 --pmc "
                                "passes over tools/sharded_one.py), mean of the two hops' launches; null when "
                                "no such file matches this batch / graph",
                "algorithmic_bytes_per_launch": round(sum(k1_bytes) / len(k1_bytes), 1),
                "avg_launch_ms": round(sum(k1_ms) / len(k1_ms), 4),
                "launch_ms": [round(x, 4) for x in k1_ms],
                "launches_per_step": phases,
                "per_rank": per_rank,
                "note": "the K1 launches of one sharded step, each timed alone on one stream with HIP "
                        "events (10 calls): hop 1 over the distinct roots, hop 2 over the distinct hop-1 "
                        "samples; bytes = SURVEY 8(d)'s K1 formula over those ids; N ranks: the mean of the "
                        "ranks' fractions, per_rank lists them",
            }

    small = None
    if rank == 0 and world == 1 and not sharded and args.full and not args.no_small_batch:
        try:
            small = latency_small_batch(G, L, _lib, args.nodes, default_node)
        except Exception as e:              # a side measurement must not fail the bench
            small = {"error": str(e)}
    secondary = None
    if rank == 0 and world == 1 and not sharded and args.workload == "metric" and args.full \
            and not args.no_secondary:
        secondary = secondary_legs(args, G, p)
    cpu = None
    if rank == 0 and args.full and not args.no_cpu_baseline:
        # (N ranks: rank 0 alone, after the timed region - the other ranks wait in the closing
        # barrier; the reference's CPU sampler does not get faster with more GPUs)
        cpu = cpu_baseline(args)

    if rank == 0:
        line = {
            "metric": ("sampled edges/sec (whole node), 2-hop fanout=[25,10], "
                       "100M-node power-law graph") if args.workload == "metric" else
                      "sampled edges/sec, uniform SampleNeighbor fanout=[25,10], ogbn-products-shaped "
                      "CSR in one MI355X's HBM (BASELINE configs[1])",
            "value": value, "unit": "sampled edges/s",
            "n_gpus": min(world, visible),
            "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {
                "workload": ("synthetic RMAT-marginal power-law graph, %d nodes / "
                             "%d edges (min degree 1), f32 weights uniform [0.5,8), "
                             "weighted CDF-inversion SampleNeighbor, fanout [25,10], "
                             "%d uniform-random roots per step per GPU, TF dense "
                             "layout" if weighted else
                             "products: synthetic power-law graph with ogbn-products' node / edge "
                             "counts, %d nodes / %d edges, all weights 1.0 (the draw is edge "
                             "floor(u * deg): no search), fanout [25,10], %d uniform-random roots "
                             "per step, TF dense layout") % (args.nodes, G.num_edges * 1 if world == 1
                                                            else args.edges, B),
                "roots_per_step_per_gpu": B, "fanout": FANOUT,
                "graph_bytes_per_gpu": G.device_bytes,
                "graph_build_s": round(build_s, 2),
                "partitioning": ("none" if not sharded else
                                 "sharded sampler on 1 rank, %d minibatches in flight" % args.pipeline)
                                if world == 1 else
                                ("replicas: every rank holds the whole graph, no exchange" if replicas else
                                 "hash owner(id)=id%%%d, all-to-all per hop, %d minibatches "
                                 "in flight" % (world, args.pipeline)),
                "replicas": replicas_leg,
                "parity_checked_edges": checked,
                "small_batch": small,
                "sustained": sustained,
                "secondary": secondary,
                "latency_B1024_us": (small or {}).get("latency_B1024_us"),
                "streams": 1 if sharded else max(1, args.streams),
                "tuning": args.tuning or None,
                "one_stream_ms_per_step": (round(float(np.median(one_stream)) / args.steps * 1e3, 4)
                                           if (not sharded and one_stream) else None),
                "repeats": len(rep_secs),
                "full": bool(args.full),
                "repeat_ms_per_step": [round(x / args.steps * 1e3, 4) for x in rep_secs],
                "ranks": world,
                "transport": (None if not (sharded or world > 1) else
                              "RCCL (torch.distributed nccl backend), %d ranks in the communicator%s"
                              % (dist.get_world_size(), "" if sharded else "; barriers and the timing "
                                 "reduction only (replicas)")
                              if backend == "nccl" else
                              "gloo, host-staged: %d ranks share %d GPU(s) - functional check, "
                              "NOT a scaling number" % (world, visible)),
                "exchanged_bytes_per_step": exchanged,
            },
            "roofline": roofline, "cpu_baseline": cpu,
            # (top level, where a parser that drops `config` still sees them: VERDICT r5 #9)
            "sustained": sustained,
            "repeat_ms_per_step": {"min": round(min(rep_secs) / args.steps * 1e3, 4),
                                   "median": round(float(np.median(rep_secs)) / args.steps * 1e3, 4),
                                   "max": round(max(rep_secs) / args.steps * 1e3, 4), "repeats": len(rep_secs)},
            "parity_checked_edges": checked,
        }
        hb = (secondary or {}).get("host_boundary")
        if isinstance(hb, dict) and "value" in hb:
            # PCIe-inclusive (host tensors on both sides of euler::Query): NOT the headline
            line["host_boundary"] = {"value": hb["value"], "unit": hb["unit"], "ms_per_step": hb["ms_per_step"],
                                     "link_only_ms_per_step": hb["device_step_plus_copy_to_pinned"]["ms_per_step"]}
        _emit(line)
    _teardown(sharded or world > 1)


if __name__ == "__main__":
    main()
