"""The errors ops.aggregate_dense raises before it touches a device or loads the library: every rule of its
argument ladder, on CPU tensors (a call that passed them all would end in the no-CPU-path RuntimeError); the
tile plan of mp_dense.h, compiled with the host compiler alone, at the boundaries the header states; and the
argument ladder of euler_gpu_aggregate_dense through the C ABI without a GPU, as test_pool_aggregate_host.py
does for its entry."""
import ctypes as C
import importlib.util
import json
import os
import shutil
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

Z = torch.zeros
BF = torch.bfloat16
BAD = [
    (dict(op="max"), ValueError), (dict(activation="tanh"), ValueError), (dict(combine="mul"), ValueError),
    (dict(table=Z(6, 8, dtype=torch.float64)), TypeError), (dict(out_dtype=torch.float16), TypeError),
    (dict(table=Z(8)), ValueError), (dict(table=Z(0, 8)), ValueError), (dict(weight=Z(7, 4)), ValueError),
    (dict(weight=Z(8, 4, dtype=BF)), ValueError), (dict(weight=Z(8, 4097)), ValueError),
    (dict(table=Z(6, 1025), weight=Z(1025, 4)), ValueError), (dict(size=-1), ValueError),
    (dict(root=None), ValueError), (dict(root=None, root_weight=None, root_scale=2.0), ValueError),
    (dict(root=None, root_weight=None, combine="fold"), ValueError), (dict(root=None, root_weight=None, combine="concat"), ValueError),
    (dict(root=Z(3)), ValueError), (dict(root=Z(4, 5)), ValueError), (dict(root=Z(3, 5, dtype=BF)), ValueError),
    (dict(root_weight=None), ValueError), (dict(root_weight=Z(6, 4)), ValueError), (dict(root_weight=Z(5, 4, dtype=BF)), ValueError),
    (dict(root_weight=Z(5, 3)), ValueError), (dict(root_scale=1.0), ValueError),
    (dict(root=Z(3, 1025), root_weight=Z(1025, 4)), ValueError), (dict(combine="concat", root_weight=Z(5, 4097)), ValueError),
    (dict(combine="fold"), ValueError), (dict(combine="fold", root_weight=None), ValueError),
    (dict(combine="fold", root_weight=None, root=Z(3, 8), root_scale=float("inf")), ValueError),
    (dict(bias=Z(5)), ValueError), (dict(bias=Z(4, dtype=torch.float16)), ValueError),
    (dict(count=None), ValueError), (dict(seg_ptr=Z(4, dtype=torch.int64)), ValueError),
    (dict(count=None, seg_ptr=Z(3, dtype=torch.int64)), ValueError), (dict(gather_indices=Z(6)), ValueError),
    (dict(count=0), ValueError), (dict(count=3), ValueError),
    # every rule passed: only now is a device asked for
    ({}, RuntimeError), (dict(root=None, root_weight=None), RuntimeError), (dict(combine="fold", root_weight=None, root=Z(3, 8), root_scale=1.5), RuntimeError),
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_python_side_errors(i):
    from euler_amd import ops
    change, error = BAD[i]
    kw = dict(op="mean", table=Z(6, 8), weight=Z(8, 4), gather_indices=Z(6, dtype=torch.int64), size=3, root=Z(3, 5),
              root_weight=Z(5, 4), bias=Z(4), count=2)
    kw.update(change)
    with pytest.raises(error):
        ops.aggregate_dense(kw.pop("op"), kw.pop("table"), kw.pop("weight"), kw.pop("gather_indices"), kw.pop("size"), **kw)


# (d, rows of root_weight | 0, max(F, Fs), fp32) -> (NT, F passes, W tiles, stride_n, stride_s, LDS bytes): mp_dense.h
PLANS = [
    # both paths 16-bit: NT 8 | 4 | 2 | 1 at d = ds = 128 | 129, 256 | 257, 512 | 513; packed columns fill 64 KB exactly
    ((128, 128, 128, 0), (8, 1, 1, 256, 256, 65536)), ((129, 129, 130, 0), (4, 3, 1, 336, 336, 43008)),
    ((256, 256, 40, 0), (4, 1, 1, 512, 512, 65536)), ((257, 257, 40, 0), (2, 2, 1, 592, 592, 37888)),
    ((512, 512, 20, 0), (2, 1, 1, 1024, 1024, 65536)), ((513, 513, 20, 0), (1, 2, 1, 1104, 1104, 35328)),
    ((1024, 1024, 17, 0), (1, 2, 1, 2048, 2048, 65536)),
    # NT by F alone: 1 | 2 | 4 | 8 at F 16 | 17, 32 | 33, 64 | 65 (d = 64: padded columns of 144 bytes)
    ((64, 0, 16, 0), (1, 1, 1, 144, 0, 2304)), ((64, 0, 17, 0), (2, 1, 1, 144, 0, 4608)),
    ((64, 0, 32, 0), (2, 1, 1, 144, 0, 4608)), ((64, 0, 33, 0), (4, 1, 1, 144, 0, 9216)),
    ((64, 0, 64, 0), (4, 1, 1, 144, 0, 9216)), ((64, 0, 65, 0), (8, 1, 1, 144, 0, 18432)),
    ((64, 0, 4096, 0), (8, 32, 1, 144, 0, 18432)),
    # fp32: free up to d = ds = 512, lockstep W tiles of 512 beyond; the neighbour path alone always fits
    ((512, 512, 16, 1), (1, 1, 1, 2048, 2048, 65536)), ((513, 512, 17, 1), (1, 2, 2, 2048, 2048, 65536)),
    ((544, 512, 16, 1), (1, 1, 2, 2048, 2048, 65536)), ((1024, 1000, 16, 1), (1, 1, 2, 2048, 2048, 65536)),
    ((1024, 0, 16, 1), (1, 1, 1, 4096, 0, 65536)), ((128, 128, 128, 1), (4, 2, 1, 512, 512, 65536)),
]


@pytest.fixture(scope="module")
def plan_lib():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so, src = os.path.join(out_dir, "libdense_plan_check.so"), os.path.join(HERE, "csrc", "dense_plan_check.cc")
    deps = [src, os.path.join(ROOT, "euler_amd", "csrc", "mp_dense.h"), os.path.join(ROOT, "euler_amd", "csrc", "mp_pool.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "euler_amd", "csrc"),
                               src, "-o", so])
    L = C.CDLL(so)
    L.dense_plan.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_int32)]
    return L


@pytest.mark.parametrize("shape,want", PLANS, ids=["-".join(map(str, s)) for s, _ in PLANS])
def test_plan_boundaries(plan_lib, shape, want):
    out = (C.c_int32 * 7)()
    plan_lib.dense_plan(*shape, out)
    nt, passes, w_tile, w_tiles, stride_n, stride_s, lds = list(out)
    assert (nt, passes, w_tiles, stride_n, stride_s, lds) == want
    assert lds <= 65536 and w_tile % 128 == 0 and (w_tiles == 1 or w_tile == 512)


T, W, B, G, S, R, RW, O = [0x1000 * (i + 1) for i in range(8)]
NAMES = ["op", "act", "combine", "table", "dtype", "rows", "weight", "bias", "bias_dtype", "gather", "is_ids", "seg_ptr",
         "count", "e", "d", "f", "size", "root", "root_weight", "ds", "fs", "has_scale", "scale", "out", "out_dtype"]
ABI = dict(op=1, act=0, combine=1, table=T, dtype=0, rows=10, weight=W, bias=B, bias_dtype=0, gather=G, is_ids=0,
           seg_ptr=None, count=2, e=8, d=12, f=5, size=4, root=R, root_weight=RW, ds=6, fs=5, has_scale=0, scale=0.0, out=O,
           out_dtype=0)
FOLD = dict(combine=3, root_weight=None, ds=12)
ALIGN = "a buffer is not aligned to its type"
PAIRING = "root goes with add, concat and fold, root_weight with add and concat"
ROWS = [
    (dict(op=0), -1, "op is 1 mean, 2 add"), (dict(op=3), -1, "op is 1 mean, 2 add"),
    (dict(act=2), -1, "activation is 0 relu, 1 none"), (dict(combine=4), -1, "combine is 0 none, 1 add, 2 concat, 3 fold"),
    (dict(dtype=3), -1, "unknown dtype (0 fp32, 1 bf16, 2 fp16)"), (dict(out_dtype=1), -1, "out is fp32 or of the table's dtype"),
    (dict(dtype=1, bias_dtype=2), -1, "bias is fp32 or of the table's dtype"), (dict(size=-1), -1, "size, e or count < 0"),
    (dict(seg_ptr=S, count=0, e=1 << 31), -1, "e or size >= 2^31"),
    (dict(d=0), -1, "d outside 1..1024 or F outside 1..4096"), (dict(d=1025), -1, "d outside 1..1024 or F outside 1..4096"),
    (dict(f=4097, fs=4097), -1, "d outside 1..1024 or F outside 1..4096"),
    (dict(ds=1025), -1, "ds outside 1..1024 or Fs outside 1..4096"), (dict(combine=2, fs=0), -1, "ds outside 1..1024 or Fs outside 1..4096"),
    (dict(fs=4), -1, "combine add needs Fs == F"), (dict(FOLD, ds=6), -1, "combine fold needs ds == d"),
    (dict(count=0), -1, "exactly one of seg_ptr and count"), (dict(seg_ptr=S), -1, "exactly one of seg_ptr and count"),
    (dict(e=9), -1, "count needs e == size * count"),
    (dict(size=0, e=0), 0, None), (dict(size=0, e=0, table=None, weight=None, root=None, root_weight=None, out=None), 0, None),
    (dict(table=None), -1, "null buffer"), (dict(out=None), -1, "null buffer"),
    (dict(root=None), -1, PAIRING), (dict(root_weight=None), -1, PAIRING), (dict(combine=0), -1, PAIRING),
    (dict(FOLD, root_weight=RW), -1, PAIRING), (dict(rows=0), -1, "a table with fewer than 1 row"),
    (dict(table=T + 2), -1, ALIGN), (dict(root=R + 2), -1, ALIGN), (dict(root_weight=RW + 2), -1, ALIGN),
    (dict(dtype=2, out_dtype=2, out=O + 1), -1, ALIGN), (dict(is_ids=1, gather=G + 4), -1, ALIGN),
]


def _answer_all():
    """(child) every row's call -> [[rc, last error], ...] on stdout"""
    spec = importlib.util.spec_from_file_location("_lib", os.path.join(ROOT, "euler_amd", "_lib.py"))
    _lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(_lib)             # (the binding alone: the package would import torch)
    L = _lib.lib()
    answers = []
    for change, _, _ in ROWS:
        v = dict(ABI, **change)
        rc = L.euler_gpu_aggregate_dense(None, *[v[n] for n in NAMES])
        answers.append([rc, L.euler_gpu_last_error().decode()])
    print(json.dumps(answers))


@pytest.fixture(scope="module")
def answers():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    return json.loads(run.stdout.decode().strip().splitlines()[-1])


@pytest.mark.parametrize("i", range(len(ROWS)))
def test_abi_row(answers, i):
    change, rc, text = ROWS[i]
    assert set(change) <= set(NAMES)
    assert answers[i][0] == rc, (change, answers[i])
    if rc != 0:
        assert answers[i][1] == "aggregate_dense: " + text, change


if __name__ == "__main__":
    _answer_all()
