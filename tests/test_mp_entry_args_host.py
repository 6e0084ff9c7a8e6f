"""The argument ladder of the sixteen segment-reduce entries (scatter_add / _max / _mean,
gather_scatter, gather_segment_reduce, gather_segment_reduce_ids, their typed `_t`, edge-weighted
`_w` and `_w_t` forms), driven through the C ABI without a GPU: return code and the full
last-error text of every call that breaks one rule.

The ladder is host arithmetic in front of the first HIP call (CheckMpReduce, mp_kernels.hip), and
libeuler_gpu.so loads without a device, so the pointers here are made-up addresses that nothing
dereferences.  EVERY row stops inside the ladder or at its `size == 0 || d == 0` early-out; none may
reach a launch.  The calls are made in one child process that sees no GPU, so that a row which a
later change lets through ends in a HIP error (rc -3, a failed row) and not in a kernel reading
address 0x1000 on a device.

A row: (entries, changes to the base call, rc, text[, what the commit before the single ladder
answered]).  The base call is valid: 8 updates, d 12, 4 destinations, count 2, mode 0, one head, a
10-row table, every pointer set but seg_ptr.  A typed entry runs a row as fp32 and as bf16 unless
the row sets in_dtype itself.  The rows with a fifth element are the three places where the single
ladder answers differently: (a) gather_scatter names itself in the messages its
scatter stage used to raise as `scatter:`, (b) a mean over e >= 2^24 updates and (c) a null gather
pointer of gather_scatter are no longer refused when there is nothing to write."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P, K, G, O, W = 0x1000, 0x2000, 0x3000, 0x5000, 0x6000     # params, scatter keys, gather, out, weights
BASE = dict(mode=0, params=P, keys=K, gather=G, seg_ptr=None, out=O, w=W, e=8, d=12, size=4, count=2,
            heads=1, params_rows=10)

_SC = ["params", "keys", "e", "d", "size", "out"]
_GS = ["mode", "params", "gather", "keys", "e", "d", "size", "out"]
_SR = ["mode", "params", "gather", "seg_ptr", "count", "d", "size", "out"]
_SRI = ["mode", "params", "params_rows", "gather", "seg_ptr", "count", "d", "size", "out"]


def _typed(args):
    """the `_t` form of an argument list: params is followed by in_dtype, out by out_dtype"""
    a = list(args)
    a.insert(a.index("params") + 1, "in_dtype")
    return a + ["out_dtype"]


ARGS = {
    "scatter_add": _SC, "scatter_max": _SC, "scatter_mean": _SC,
    "scatter_t": _typed(["mode"] + _SC),
    "gather_scatter": _GS, "gather_scatter_t": _typed(_GS),
    "gather_segment_reduce": _SR, "gather_segment_reduce_t": _typed(_SR),
    "gather_segment_reduce_ids": _SRI, "gather_segment_reduce_ids_t": _typed(_SRI),
    "gather_scatter_w": _GS + ["w", "heads"], "gather_scatter_w_t": _typed(_GS) + ["w", "w_dtype", "heads"],
    "gather_segment_reduce_w": _SR + ["w", "heads"],
    "gather_segment_reduce_w_t": _typed(_SR) + ["w", "w_dtype", "heads"],
    "gather_segment_reduce_ids_w": _SRI + ["w", "heads"],
    "gather_segment_reduce_ids_w_t": _typed(_SRI) + ["w", "w_dtype", "heads"],
}

SC_F32 = ("scatter_add", "scatter_max", "scatter_mean")
SC = SC_F32 + ("scatter_t",)
GS = ("gather_scatter", "gather_scatter_t")
SR = ("gather_segment_reduce", "gather_segment_reduce_t")
SRI = ("gather_segment_reduce_ids", "gather_segment_reduce_ids_t")
GSW = ("gather_scatter_w", "gather_scatter_w_t")
SRW = ("gather_segment_reduce_w", "gather_segment_reduce_w_t")
SRIW = ("gather_segment_reduce_ids_w", "gather_segment_reduce_ids_w_t")

BF16 = dict(in_dtype=1, out_dtype=1)
E24, E31 = 1 << 24, 1 << 31

ROWS = [
    # ---- scatter_add / scatter_max / scatter_mean / scatter_t --------------------------------
    (("scatter_t",), dict(mode=-1), -1, "scatter: mode is 0 add, 1 max, 2 mean"),
    (("scatter_t",), dict(mode=3), -1, "scatter: mode is 0 add, 1 max, 2 mean"),
    (("scatter_t",), dict(in_dtype=7, out_dtype=0), -1, "scatter: unknown dtype 7 (0 fp32, 1 bf16, 2 fp16)"),
    (("scatter_t",), dict(in_dtype=-1, out_dtype=0), -1, "scatter: unknown dtype -1 (0 fp32, 1 bf16, 2 fp16)"),
    (("scatter_t",), dict(in_dtype=1, out_dtype=2), -1, "scatter: out_dtype 2 is neither fp32 nor the input's dtype"),
    (("scatter_t",), dict(in_dtype=0, out_dtype=1), -1, "scatter: out_dtype 1 is neither fp32 nor the input's dtype"),
    (SC, dict(e=-1), -1, "scatter: bad shape"),
    (SC, dict(d=-1), -1, "scatter: bad shape"),
    (SC, dict(size=-1), -1, "scatter: bad shape"),
    (SC, dict(size=0), 0, None),
    (SC, dict(d=0), 0, None),
    (SC, dict(out=None), -1, "scatter: null buffer"),
    (SC, dict(params=None), -1, "scatter: null buffer"),
    (SC, dict(keys=None), -1, "scatter: null buffer"),
    (("scatter_add", "scatter_max", "scatter_t"), dict(e=E31), -1, "scatter: e >= 2^31"),
    (("scatter_mean",), dict(e=E24), -1, "scatter_mean: e >= 2^24, compose scatter_add instead"),
    (("scatter_t",), dict(mode=2, e=E24), -1, "scatter_mean: e >= 2^24, compose scatter_add instead"),
    (("scatter_t",), dict(BF16, params=P + 1), -1, "scatter: 16-bit data must be 2-byte aligned"),
    (("scatter_t",), dict(BF16, out=O + 1), -1, "scatter: 16-bit data must be 2-byte aligned"),
    (("scatter_t",), dict(in_dtype=2, out_dtype=0, out=O + 1), -1, "scatter: 16-bit data must be 2-byte aligned"),
    # (b)
    (("scatter_mean",), dict(e=E24, size=0), 0, None,
     (-1, "scatter_mean: e >= 2^24, compose scatter_add instead")),
    (("scatter_mean",), dict(e=E24, d=0), 0, None,
     (-1, "scatter_mean: e >= 2^24, compose scatter_add instead")),
    (("scatter_t",), dict(mode=2, e=E24, size=0), 0, None,
     (-1, "scatter_mean: e >= 2^24, compose scatter_add instead")),
    (("scatter_t",), dict(mode=2, e=E24, d=0), 0, None,
     (-1, "scatter_mean: e >= 2^24, compose scatter_add instead")),

    # ---- gather_scatter / gather_scatter_t ---------------------------------------------------
    (GS, dict(mode=-1), -1, "gather_scatter: mode is 0 add, 1 max, 2 mean"),
    (GS, dict(mode=3), -1, "gather_scatter: mode is 0 add, 1 max, 2 mean"),
    (GS[1:], dict(in_dtype=7, out_dtype=0), -1, "gather_scatter: unknown dtype 7 (0 fp32, 1 bf16, 2 fp16)"),
    (GS[1:], dict(in_dtype=-1, out_dtype=0), -1, "gather_scatter: unknown dtype -1 (0 fp32, 1 bf16, 2 fp16)"),
    (GS[1:], dict(in_dtype=2, out_dtype=1), -1,
     "gather_scatter: out_dtype 1 is neither fp32 nor the input's dtype"),
    (GS[1:], dict(in_dtype=0, out_dtype=2), -1,
     "gather_scatter: out_dtype 2 is neither fp32 nor the input's dtype"),
    (GS, dict(size=0), 0, None),
    (GS, dict(d=0), 0, None),
    (GS, dict(gather=None), -1, "gather_scatter: null buffer"),
    (GS, dict(mode=2, e=E24), -1, "gather_scatter: mean needs e < 2^24"),
    # (a)
    (GS, dict(e=-1), -1, "gather_scatter: bad shape", (-1, "scatter: bad shape")),
    (GS, dict(d=-1), -1, "gather_scatter: bad shape", (-1, "scatter: bad shape")),
    (GS, dict(size=-1), -1, "gather_scatter: bad shape", (-1, "scatter: bad shape")),
    (GS, dict(out=None), -1, "gather_scatter: null buffer", (-1, "scatter: null buffer")),
    (GS, dict(params=None), -1, "gather_scatter: null buffer", (-1, "scatter: null buffer")),
    (GS, dict(keys=None), -1, "gather_scatter: null buffer", (-1, "scatter: null buffer")),
    (GS, dict(e=E31), -1, "gather_scatter: e >= 2^31", (-1, "scatter: e >= 2^31")),
    (GS[1:], dict(BF16, params=P + 1), -1, "gather_scatter: 16-bit data must be 2-byte aligned",
     (-1, "scatter: 16-bit data must be 2-byte aligned")),
    (GS[1:], dict(BF16, out=O + 1), -1, "gather_scatter: 16-bit data must be 2-byte aligned",
     (-1, "scatter: 16-bit data must be 2-byte aligned")),
    # (b)
    (GS, dict(mode=2, e=E24, size=0), 0, None, (-1, "gather_scatter: mean needs e < 2^24")),
    (GS, dict(mode=2, e=E24, d=0), 0, None, (-1, "gather_scatter: mean needs e < 2^24")),
    # (c)
    (GS, dict(gather=None, size=0), 0, None, (-1, "gather_scatter: null buffer")),
    (GS, dict(gather=None, d=0), 0, None, (-1, "gather_scatter: null buffer")),

    # ---- gather_segment_reduce / _t ----------------------------------------------------------
    (SR, dict(mode=-1), -1, "gather_segment_reduce: mode is 0 add, 1 max, 2 mean"),
    (SR, dict(mode=3), -1, "gather_segment_reduce: mode is 0 add, 1 max, 2 mean"),
    (SR[1:], dict(in_dtype=7, out_dtype=0), -1, "gather_segment_reduce: unknown dtype 7 (0 fp32, 1 bf16, 2 fp16)"),
    (SR[1:], dict(in_dtype=-1, out_dtype=0), -1, "gather_segment_reduce: unknown dtype -1 (0 fp32, 1 bf16, 2 fp16)"),
    (SR[1:], dict(in_dtype=1, out_dtype=2), -1,
     "gather_segment_reduce: out_dtype 2 is neither fp32 nor the input's dtype"),
    (SR[1:], dict(in_dtype=0, out_dtype=1), -1,
     "gather_segment_reduce: out_dtype 1 is neither fp32 nor the input's dtype"),
    (SR, dict(d=-1), -1, "gather_segment_reduce: bad shape"),
    (SR, dict(size=-1), -1, "gather_segment_reduce: bad shape"),
    (SR, dict(count=-1), -1, "gather_segment_reduce: bad shape"),
    (SR, dict(size=0), 0, None),
    (SR, dict(d=0), 0, None),
    (SR, dict(out=None), -1, "gather_segment_reduce: null buffer"),
    (SR, dict(params=None), -1, "gather_segment_reduce: null buffer"),
    (SR, dict(mode=2, count=E24), -1, "gather_segment_reduce: mean needs segments shorter than 2^24"),
    (SR[1:], dict(BF16, params=P + 1), -1, "gather_segment_reduce: 16-bit data must be 2-byte aligned"),
    (SR[1:], dict(BF16, out=O + 1), -1, "gather_segment_reduce: 16-bit data must be 2-byte aligned"),

    # ---- gather_segment_reduce_ids / _ids_t --------------------------------------------------
    (SRI, dict(mode=-1), -1, "gather_segment_reduce_ids: mode is 0 add, 1 max, 2 mean"),
    (SRI, dict(mode=3), -1, "gather_segment_reduce_ids: mode is 0 add, 1 max, 2 mean"),
    (SRI[1:], dict(in_dtype=7, out_dtype=0), -1,
     "gather_segment_reduce_ids: unknown dtype 7 (0 fp32, 1 bf16, 2 fp16)"),
    (SRI[1:], dict(in_dtype=-1, out_dtype=0), -1,
     "gather_segment_reduce_ids: unknown dtype -1 (0 fp32, 1 bf16, 2 fp16)"),
    (SRI[1:], dict(in_dtype=1, out_dtype=2), -1,
     "gather_segment_reduce_ids: out_dtype 2 is neither fp32 nor the input's dtype"),
    (SRI[1:], dict(in_dtype=0, out_dtype=1), -1,
     "gather_segment_reduce_ids: out_dtype 1 is neither fp32 nor the input's dtype"),
    (SRI, dict(d=-1), -1, "gather_segment_reduce_ids: bad shape"),
    (SRI, dict(size=-1), -1, "gather_segment_reduce_ids: bad shape"),
    (SRI, dict(count=-1), -1, "gather_segment_reduce_ids: bad shape"),
    (SRI, dict(size=0), 0, None),
    (SRI, dict(d=0), 0, None),
    (SRI, dict(out=None), -1, "gather_segment_reduce_ids: null buffer"),
    (SRI, dict(params=None), -1, "gather_segment_reduce_ids: null buffer"),
    (SRI, dict(gather=None), -1, "gather_segment_reduce_ids: null buffer"),
    (SRI, dict(mode=2, count=E24), -1, "gather_segment_reduce_ids: mean needs segments shorter than 2^24"),
    (SRI, dict(params_rows=E31), -1, "gather_segment_reduce_ids: the table must have fewer than 2^31 rows"),
    (SRI, dict(params_rows=-1), -1, "gather_segment_reduce_ids: the table must have fewer than 2^31 rows"),
    (SRI[1:], dict(BF16, params=P + 1), -1, "gather_segment_reduce_ids: 16-bit data must be 2-byte aligned"),
    (SRI[1:], dict(BF16, out=O + 1), -1, "gather_segment_reduce_ids: 16-bit data must be 2-byte aligned"),

    # ---- gather_scatter_w / _w_t -------------------------------------------------------------
    (GSW, dict(mode=-1), -1, "gather_scatter_w: mode is 0 add, 1 max, 2 mean"),
    (GSW, dict(mode=3), -1, "gather_scatter_w: mode is 0 add, 1 max, 2 mean"),
    (GSW, dict(heads=0), -1, "gather_scatter_w: heads < 1"),
    (GSW, dict(heads=5), -1, "gather_scatter_w: heads must divide d"),
    (GSW, dict(d=-1), -1, "gather_scatter_w: heads must divide d"),
    (GSW[1:], dict(in_dtype=7, out_dtype=0, w_dtype=0), -1,
     "gather_scatter_w: unknown dtype 7 (0 fp32, 1 bf16, 2 fp16)"),
    (GSW[1:], dict(in_dtype=-1, out_dtype=0, w_dtype=0), -1,
     "gather_scatter_w: unknown dtype -1 (0 fp32, 1 bf16, 2 fp16)"),
    (GSW[1:], dict(in_dtype=1, out_dtype=2, w_dtype=0), -1,
     "gather_scatter_w: out_dtype 2 is neither fp32 nor the input's dtype"),
    (GSW[1:], dict(in_dtype=0, out_dtype=1, w_dtype=0), -1,
     "gather_scatter_w: out_dtype 1 is neither fp32 nor the input's dtype"),
    (GSW[1:], dict(in_dtype=1, out_dtype=1, w_dtype=2), -1,
     "gather_scatter_w: w_dtype 2 is neither fp32 nor the input's dtype"),
    (GSW[1:], dict(in_dtype=0, out_dtype=0, w_dtype=1), -1,
     "gather_scatter_w: w_dtype 1 is neither fp32 nor the input's dtype"),
    (GSW[1:], dict(w=W + 2), -1, "gather_scatter_w: the weights are not aligned to their type"),
    (GSW[1:], dict(BF16, w_dtype=1, w=W + 1), -1, "gather_scatter_w: the weights are not aligned to their type"),
    (GSW, dict(e=-1), -1, "gather_scatter_w: bad shape"),
    (GSW, dict(size=-1), -1, "gather_scatter_w: bad shape"),
    (GSW, dict(size=0), 0, None),
    (GSW, dict(d=0), 0, None),
    (GSW, dict(out=None), -1, "gather_scatter_w: null buffer"),
    (GSW, dict(params=None), -1, "gather_scatter_w: null buffer"),
    (GSW, dict(keys=None), -1, "gather_scatter_w: null buffer"),
    (GSW, dict(w=None), -1, "gather_scatter_w: null buffer"),
    (GSW, dict(e=E31), -1, "gather_scatter_w: e >= 2^31"),
    (GSW, dict(mode=2, e=E24), -1, "gather_scatter_w: mean needs e < 2^24"),
    (GSW, dict(mode=2, e=E24, size=0), 0, None),
    (GSW[1:], dict(BF16, params=P + 1), -1, "gather_scatter_w: 16-bit data must be 2-byte aligned"),
    (GSW[1:], dict(BF16, out=O + 1), -1, "gather_scatter_w: 16-bit data must be 2-byte aligned"),

    # ---- gather_segment_reduce_w / _w_t ------------------------------------------------------
    (SRW, dict(mode=-1), -1, "gather_segment_reduce_w: mode is 0 add, 1 max, 2 mean"),
    (SRW, dict(mode=3), -1, "gather_segment_reduce_w: mode is 0 add, 1 max, 2 mean"),
    (SRW, dict(heads=0), -1, "gather_segment_reduce_w: heads < 1"),
    (SRW, dict(heads=5), -1, "gather_segment_reduce_w: heads must divide d"),
    (SRW, dict(d=-1), -1, "gather_segment_reduce_w: heads must divide d"),
    (SRW[1:], dict(in_dtype=7, out_dtype=0, w_dtype=0), -1,
     "gather_segment_reduce_w: unknown dtype 7 (0 fp32, 1 bf16, 2 fp16)"),
    (SRW[1:], dict(in_dtype=-1, out_dtype=0, w_dtype=0), -1,
     "gather_segment_reduce_w: unknown dtype -1 (0 fp32, 1 bf16, 2 fp16)"),
    (SRW[1:], dict(in_dtype=1, out_dtype=2, w_dtype=0), -1,
     "gather_segment_reduce_w: out_dtype 2 is neither fp32 nor the input's dtype"),
    (SRW[1:], dict(in_dtype=0, out_dtype=1, w_dtype=0), -1,
     "gather_segment_reduce_w: out_dtype 1 is neither fp32 nor the input's dtype"),
    (SRW[1:], dict(in_dtype=1, out_dtype=1, w_dtype=2), -1,
     "gather_segment_reduce_w: w_dtype 2 is neither fp32 nor the input's dtype"),
    (SRW[1:], dict(in_dtype=0, out_dtype=0, w_dtype=1), -1,
     "gather_segment_reduce_w: w_dtype 1 is neither fp32 nor the input's dtype"),
    (SRW[1:], dict(w=W + 2), -1, "gather_segment_reduce_w: the weights are not aligned to their type"),
    (SRW[1:], dict(BF16, w_dtype=1, w=W + 1), -1,
     "gather_segment_reduce_w: the weights are not aligned to their type"),
    (SRW, dict(size=-1), -1, "gather_segment_reduce_w: bad shape"),
    (SRW, dict(count=-1), -1, "gather_segment_reduce_w: bad shape"),
    (SRW, dict(size=0), 0, None),
    (SRW, dict(d=0), 0, None),
    (SRW, dict(out=None), -1, "gather_segment_reduce_w: null buffer"),
    (SRW, dict(params=None), -1, "gather_segment_reduce_w: null buffer"),
    (SRW, dict(w=None), -1, "gather_segment_reduce_w: null buffer"),
    (SRW, dict(size=2, count=1 << 30), -1, "gather_segment_reduce_w: e >= 2^31"),
    (SRW, dict(mode=2, count=E24), -1, "gather_segment_reduce_w: mean needs segments shorter than 2^24"),
    (SRW[1:], dict(BF16, params=P + 1), -1, "gather_segment_reduce_w: 16-bit data must be 2-byte aligned"),
    (SRW[1:], dict(BF16, out=O + 1), -1, "gather_segment_reduce_w: 16-bit data must be 2-byte aligned"),

    # ---- gather_segment_reduce_ids_w / _ids_w_t ----------------------------------------------
    (SRIW, dict(mode=-1), -1, "gather_segment_reduce_ids_w: mode is 0 add, 1 max, 2 mean"),
    (SRIW, dict(mode=3), -1, "gather_segment_reduce_ids_w: mode is 0 add, 1 max, 2 mean"),
    (SRIW, dict(heads=0), -1, "gather_segment_reduce_ids_w: heads < 1"),
    (SRIW, dict(heads=5), -1, "gather_segment_reduce_ids_w: heads must divide d"),
    (SRIW, dict(d=-1), -1, "gather_segment_reduce_ids_w: heads must divide d"),
    (SRIW[1:], dict(in_dtype=7, out_dtype=0, w_dtype=0), -1,
     "gather_segment_reduce_ids_w: unknown dtype 7 (0 fp32, 1 bf16, 2 fp16)"),
    (SRIW[1:], dict(in_dtype=-1, out_dtype=0, w_dtype=0), -1,
     "gather_segment_reduce_ids_w: unknown dtype -1 (0 fp32, 1 bf16, 2 fp16)"),
    (SRIW[1:], dict(in_dtype=1, out_dtype=2, w_dtype=0), -1,
     "gather_segment_reduce_ids_w: out_dtype 2 is neither fp32 nor the input's dtype"),
    (SRIW[1:], dict(in_dtype=0, out_dtype=1, w_dtype=0), -1,
     "gather_segment_reduce_ids_w: out_dtype 1 is neither fp32 nor the input's dtype"),
    (SRIW[1:], dict(in_dtype=1, out_dtype=1, w_dtype=2), -1,
     "gather_segment_reduce_ids_w: w_dtype 2 is neither fp32 nor the input's dtype"),
    (SRIW[1:], dict(in_dtype=0, out_dtype=0, w_dtype=1), -1,
     "gather_segment_reduce_ids_w: w_dtype 1 is neither fp32 nor the input's dtype"),
    (SRIW[1:], dict(w=W + 2), -1, "gather_segment_reduce_ids_w: the weights are not aligned to their type"),
    (SRIW[1:], dict(BF16, w_dtype=1, w=W + 1), -1,
     "gather_segment_reduce_ids_w: the weights are not aligned to their type"),
    (SRIW, dict(size=-1), -1, "gather_segment_reduce_ids_w: bad shape"),
    (SRIW, dict(count=-1), -1, "gather_segment_reduce_ids_w: bad shape"),
    (SRIW, dict(size=0), 0, None),
    (SRIW, dict(d=0), 0, None),
    (SRIW, dict(out=None), -1, "gather_segment_reduce_ids_w: null buffer"),
    (SRIW, dict(params=None), -1, "gather_segment_reduce_ids_w: null buffer"),
    (SRIW, dict(gather=None), -1, "gather_segment_reduce_ids_w: null buffer"),
    (SRIW, dict(w=None), -1, "gather_segment_reduce_ids_w: null buffer"),
    (SRIW, dict(size=2, count=1 << 30), -1, "gather_segment_reduce_ids_w: e >= 2^31"),
    (SRIW, dict(mode=2, count=E24), -1, "gather_segment_reduce_ids_w: mean needs segments shorter than 2^24"),
    (SRIW, dict(params_rows=E31), -1, "gather_segment_reduce_ids_w: the table must have fewer than 2^31 rows"),
    (SRIW, dict(params_rows=-1), -1, "gather_segment_reduce_ids_w: the table must have fewer than 2^31 rows"),
    (SRIW[1:], dict(BF16, params=P + 1), -1, "gather_segment_reduce_ids_w: 16-bit data must be 2-byte aligned"),
    (SRIW[1:], dict(BF16, out=O + 1), -1, "gather_segment_reduce_ids_w: 16-bit data must be 2-byte aligned"),
]


def _cases(row):
    """the calls of a row: (entry, its argument values in ABI order)"""
    out = []
    for entry in row[0]:
        names = ARGS[entry]
        dtypes = [{}]
        if "in_dtype" in names:
            dtypes = [dict(in_dtype=0, out_dtype=0, w_dtype=0), dict(in_dtype=1, out_dtype=1, w_dtype=0)]
            if "in_dtype" in row[1]:
                dtypes = dtypes[:1]
        for dt in dtypes:
            v = dict(BASE, **dt)
            v.update(row[1])
            out.append((entry, [v[n] for n in names]))
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
            rc = getattr(L, "euler_gpu_" + entry)(None, *values)
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


def test_table_covers_every_entry():
    assert sorted(ARGS) == sorted({e for row in ROWS for e in row[0]}) and len(ARGS) == 16
    from euler_amd import _lib
    for entry, names in ARGS.items():
        assert len(_lib.SIGNATURES["euler_gpu_" + entry][1]) == 1 + len(names), entry


@pytest.mark.parametrize("i", range(len(ROWS)), ids=lambda i: "%03d-%s" % (i, ROWS[i][0][0]))
def test_row(answers, i):
    row = ROWS[i]
    # EULER_GPU_MP_ARGS_BEFORE=1: the answers of the commit before the single ladder (a build of it
    # in EULER_GPU_LIB_PATH) - the fifth element where a row has one
    want = row[4] if len(row) > 4 and os.environ.get("EULER_GPU_MP_ARGS_BEFORE") == "1" else row[2:4]
    for (entry, values), (rc, text) in zip(_cases(row), answers[i]):
        assert rc == want[0], (entry, values, rc, text)
        if want[0] != 0:
            assert text == want[1], (entry, values)


if __name__ == "__main__":
    _answer_all()
