"""The errors ops.aggregate_gru raises before it touches a device or loads the library, on CPU tensors (a call that
passed them all ends in the no-CPU-path RuntimeError); the plan of mp_gru.h, compiled with the host compiler alone,
at its boundaries; and the argument ladder of euler_gpu_aggregate_gru through the C ABI without a GPU, as
test_aggregate_dense_host.py does for its entry."""
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
    (dict(op="max"), ValueError), (dict(table=Z(6, 8, dtype=torch.float64)), ValueError), (dict(out_dtype=torch.float16), ValueError),
    (dict(table=Z(8)), ValueError), (dict(table=Z(0, 8)), ValueError), (dict(size=-1), ValueError),
    (dict(state=Z(5)), ValueError), (dict(state=Z(4, 5)), ValueError), (dict(state=Z(3, 5, dtype=BF)), ValueError),
    (dict(table=Z(6, 257), gate_weight=Z(262, 10), cand_weight=Z(262, 5)), ValueError),
    (dict(state=Z(3, 257), gate_weight=Z(265, 514), cand_weight=Z(265, 257)), ValueError),
    (dict(gate_weight=Z(13, 5)), ValueError), (dict(gate_weight=Z(12, 10)), ValueError), (dict(gate_weight=Z(13, 10, dtype=BF)), ValueError),
    (dict(cand_weight=Z(13, 10)), ValueError), (dict(cand_weight=Z(13, 5, dtype=BF)), ValueError),
    (dict(gate_bias=Z(5)), ValueError), (dict(cand_bias=Z(10)), ValueError), (dict(gate_bias=Z(10, dtype=BF)), ValueError),
    (dict(count=None), ValueError), (dict(seg_ptr=Z(4, dtype=torch.int64)), ValueError),
    (dict(count=None, seg_ptr=Z(3, dtype=torch.int64)), ValueError), (dict(gather_indices=Z(6)), ValueError),
    (dict(count=0), ValueError), (dict(count=3), ValueError),
    # every rule passed: only now is a device asked for
    ({}, RuntimeError), (dict(gate_bias=None, cand_bias=None, gather_indices=None), RuntimeError),
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_python_side_errors(i):
    from euler_amd import ops
    change, error = BAD[i]
    kw = dict(op="add", table=Z(6, 8), gather_indices=Z(6, dtype=torch.int64), size=3, state=Z(3, 5), gate_weight=Z(13, 10),
              cand_weight=Z(13, 5), gate_bias=Z(10), cand_bias=Z(5), count=2)
    kw.update(change)
    with pytest.raises(error):
        ops.aggregate_gru(kw.pop("op"), kw.pop("table"), kw.pop("gather_indices"), kw.pop("size"), kw.pop("state"), **kw)


# (d, U, fp32) -> (CH, NT, kd, ku, r passes, c passes, stride, LDS bytes): mp_gru.h
PLANS = [
    # 16 bits: CH 4 (NT 4) up to max(d, U) = 128 - d = U = 128 packed, 64 KB, 1 r pass + 2 c passes - CH 8 (NT 2) beyond
    ((128, 128, 0), (4, 4, 4, 4, 1, 2, 512, 65536)), ((129, 128, 0), (8, 2, 5, 4, 2, 4, 592, 37888)),
    ((128, 129, 0), (8, 2, 4, 5, 3, 5, 592, 37888)), ((64, 64, 0), (4, 4, 2, 2, 1, 1, 256, 32768)),
    ((64, 65, 0), (4, 4, 2, 3, 1, 2, 336, 43008)), ((1, 1, 0), (4, 4, 1, 1, 1, 1, 144, 18432)),
    ((256, 192, 0), (8, 2, 8, 6, 3, 6, 912, 58368)), ((256, 193, 0), (8, 2, 8, 7, 4, 7, 976, 62464)),
    ((8, 160, 0), (8, 2, 1, 5, 3, 5, 400, 25600)), ((8, 161, 0), (8, 2, 1, 6, 3, 6, 464, 29696)),
    ((256, 256, 0), (8, 2, 8, 8, 4, 8, 1024, 65536)),
    # fp32: CH 4 has NT 2, CH 8 has NT 1
    ((128, 128, 1), (4, 2, 4, 4, 2, 4, 1024, 65536)), ((64, 32, 1), (4, 2, 2, 1, 1, 1, 400, 25600)),
    ((64, 33, 1), (4, 2, 2, 2, 1, 2, 512, 32768)), ((64, 65, 1), (4, 2, 2, 3, 2, 3, 656, 41984)),
    ((200, 144, 1), (8, 1, 7, 5, 5, 9, 1536, 49152)), ((200, 145, 1), (8, 1, 7, 5, 5, 10, 1536, 49152)),
    ((256, 256, 1), (8, 1, 8, 8, 8, 16, 2048, 65536)),
]


@pytest.fixture(scope="module")
def plan_lib():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so, src = os.path.join(out_dir, "libgru_plan_check.so"), os.path.join(HERE, "csrc", "gru_plan_check.cc")
    deps = [src] + [os.path.join(ROOT, "euler_amd", "csrc", h) for h in ("mp_gru.h", "mp_dense.h", "mp_pool.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "euler_amd", "csrc"),
                               src, "-o", so])
    L = C.CDLL(so)
    L.gru_plan.argtypes = [C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_int32)]
    return L


@pytest.mark.parametrize("shape,want", PLANS, ids=["-".join(map(str, s)) for s, _ in PLANS])
def test_plan_boundaries(plan_lib, shape, want):
    out = (C.c_int32 * 8)()
    plan_lib.gru_plan(*shape, out)
    assert tuple(out) == want
    assert out[7] <= 65536 and out[7] == 32 * out[1] * out[6]


def test_state_row_permutation(plan_lib):
    """slot 8 g + j of chunk x holds the column tiles 2 x and 2 x + 1 gave lane group g: a permutation of 0 .. 255"""
    rows = [plan_lib.gru_state_row(s) for s in range(256)]
    assert sorted(rows) == list(range(256))
    assert all(rows[32 * x + 8 * g + j] == 32 * x + 16 * (j // 4) + 4 * g + j % 4
               for x in range(8) for g in range(4) for j in range(8))


T, H, WG, WC, BG, BC, G, S, O = [0x1000 * (i + 1) for i in range(9)]
NAMES = ["op", "table", "dtype", "rows", "gather", "is_ids", "seg_ptr", "count", "e", "d", "u", "size", "state", "gate_weight",
         "cand_weight", "gate_bias", "gate_bias_dtype", "cand_bias", "cand_bias_dtype", "out", "out_dtype"]
ABI = dict(op=2, table=T, dtype=0, rows=10, gather=G, is_ids=0, seg_ptr=None, count=2, e=8, d=12, u=5, size=4, state=H,
           gate_weight=WG, cand_weight=WC, gate_bias=BG, gate_bias_dtype=0, cand_bias=BC, cand_bias_dtype=0, out=O, out_dtype=0)
ALIGN = "a buffer is not aligned to its type"
ROWS = [
    (dict(op=0), -1, "op is 1 mean, 2 add"), (dict(op=3), -1, "op is 1 mean, 2 add"),
    (dict(dtype=3), -1, "unknown dtype (0 fp32, 1 bf16, 2 fp16)"), (dict(cand_bias_dtype=7), -1, "unknown dtype (0 fp32, 1 bf16, 2 fp16)"),
    (dict(out_dtype=1), -1, "out is fp32 or of the table's dtype"),
    (dict(dtype=1, gate_bias_dtype=2), -1, "a bias is fp32 or of the table's dtype"),
    (dict(dtype=1, cand_bias_dtype=2), -1, "a bias is fp32 or of the table's dtype"),
    (dict(size=-1), -1, "size, e or count < 0"), (dict(seg_ptr=S, count=0, e=1 << 31), -1, "e or size >= 2^31"),
    (dict(d=0), -1, "d outside 1..256 or U outside 1..256"), (dict(d=257), -1, "d outside 1..256 or U outside 1..256"),
    (dict(u=0), -1, "d outside 1..256 or U outside 1..256"), (dict(u=257), -1, "d outside 1..256 or U outside 1..256"),
    (dict(count=0), -1, "exactly one of seg_ptr and count"), (dict(seg_ptr=S), -1, "exactly one of seg_ptr and count"),
    (dict(e=9), -1, "count needs e == size * count"),
    (dict(size=0, e=0), 0, None), (dict(size=0, e=0, table=None, state=None, gate_weight=None, cand_weight=None, out=None), 0, None),
    (dict(table=None), -1, "null buffer"), (dict(state=None), -1, "null buffer"), (dict(gate_weight=None), -1, "null buffer"),
    (dict(cand_weight=None), -1, "null buffer"), (dict(out=None), -1, "null buffer"),
    (dict(rows=0), -1, "a table with fewer than 1 row"),
    (dict(table=T + 2), -1, ALIGN), (dict(state=H + 2), -1, ALIGN), (dict(cand_weight=WC + 2), -1, ALIGN),
    (dict(cand_bias=BC + 2), -1, ALIGN), (dict(dtype=2, out_dtype=2, out=O + 1), -1, ALIGN), (dict(is_ids=1, gather=G + 4), -1, ALIGN),
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
        rc = L.euler_gpu_aggregate_gru(None, *[v[n] for n in NAMES])
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
        assert answers[i][1] == "aggregate_gru: " + text, change


if __name__ == "__main__":
    _answer_all()
