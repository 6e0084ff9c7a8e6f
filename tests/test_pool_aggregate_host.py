"""The argument ladder of euler_gpu_pool_aggregate through the C ABI without a GPU, as
tests/test_segment_entry_args_host.py does for its entries (made-up addresses nothing dereferences, one
child process that sees no device); then the errors ops.pool_aggregate raises before it touches a device."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, W, B, G, S, O = [0x1000 * (i + 1) for i in range(6)]
E31 = 1 << 31
CODES = " (0 fp32, 1 bf16, 2 fp16)"
ALIGN = "a buffer is not aligned to its type"
FORM = "exactly one of seg_ptr and count"

NAMES = ["op", "act", "table", "dtype", "rows", "weight", "bias", "bias_dtype", "gather", "is_ids", "seg_ptr", "count",
         "e", "d", "f", "size", "out", "out_dtype"]
BASE = dict(op=0, act=0, table=T, dtype=0, rows=10, weight=W, bias=B, bias_dtype=0, gather=G, is_ids=0, seg_ptr=None,
            count=2, e=8, d=12, f=5, size=4, out=O, out_dtype=0)
PTR = dict(seg_ptr=S, count=0)

ROWS = [
    (dict(op=3), -1, "op is 0 max, 1 mean, 2 add"), (dict(op=-1), -1, "op is 0 max, 1 mean, 2 add"),
    (dict(act=2), -1, "activation is 0 relu, 1 none"),
    (dict(dtype=3), -1, "unknown dtype" + CODES), (dict(out_dtype=-1), -1, "unknown dtype" + CODES),
    (dict(bias_dtype=3), -1, "unknown dtype" + CODES),
    (dict(dtype=1, out_dtype=2), -1, "out is fp32 or of the table's dtype"),
    (dict(out_dtype=1), -1, "out is fp32 or of the table's dtype"),
    (dict(dtype=1, bias_dtype=2), -1, "bias is fp32 or of the table's dtype"),
    (dict(size=-1), -1, "size, e or count < 0"), (dict(e=-1), -1, "size, e or count < 0"),
    (dict(count=-1), -1, "size, e or count < 0"),
    (dict(PTR, e=E31), -1, "e or size >= 2^31"), (dict(PTR, size=E31), -1, "e or size >= 2^31"),
    (dict(d=0), -1, "d or F outside 1..4096"), (dict(d=4097), -1, "d or F outside 1..4096"),
    (dict(f=0), -1, "d or F outside 1..4096"), (dict(f=4097), -1, "d or F outside 1..4096"),
    (dict(count=0), -1, FORM), (dict(seg_ptr=S), -1, FORM),
    (dict(count=3), -1, "count needs e == size * count"), (dict(e=9), -1, "count needs e == size * count"),
    (dict(size=0, e=0), 0, None), (dict(PTR, size=0), 0, None),
    (dict(size=0, e=0, table=None, weight=None, bias=None, gather=None, out=None), 0, None),
    (dict(table=None), -1, "null buffer"), (dict(weight=None), -1, "null buffer"), (dict(out=None), -1, "null buffer"),
    (dict(rows=0), -1, "a table with fewer than 1 row"),
    (dict(table=T + 2), -1, ALIGN), (dict(dtype=1, table=T + 1), -1, ALIGN), (dict(weight=W + 2), -1, ALIGN),
    (dict(bias=B + 2), -1, ALIGN), (dict(out=O + 2), -1, ALIGN), (dict(dtype=2, out_dtype=2, out=O + 1), -1, ALIGN),
    (dict(PTR, seg_ptr=S + 4), -1, ALIGN), (dict(gather=G + 2), -1, ALIGN), (dict(is_ids=1, gather=G + 4), -1, ALIGN),
]


def _answer_all():
    """(child) every row's call -> [[rc, last error], ...] on stdout"""
    spec = importlib.util.spec_from_file_location("_lib", os.path.join(ROOT, "euler_amd", "_lib.py"))
    _lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(_lib)             # (the binding alone: the package would import torch)
    L = _lib.lib()
    answers = []
    for change, _, _ in ROWS:
        v = dict(BASE, **change)
        rc = L.euler_gpu_pool_aggregate(None, *[v[n] for n in NAMES])
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
def test_row(answers, i):
    change, rc, text = ROWS[i]
    assert set(change) <= set(NAMES)
    assert answers[i][0] == rc, (change, answers[i])
    if rc != 0:
        assert answers[i][1] == "pool_aggregate: " + text, change


def _bad():
    import torch
    z = torch.zeros
    return [
        (dict(op="min"), ValueError), (dict(activation="tanh"), ValueError),
        (dict(table=z(6, 8, dtype=torch.float64)), TypeError), (dict(out_dtype=torch.float16), TypeError),
        (dict(table=z(8)), ValueError), (dict(table=z(0, 8)), ValueError), (dict(weight=z(7, 4)), ValueError),
        (dict(weight=z(8, 4, dtype=torch.bfloat16)), ValueError), (dict(weight=z(8, 4097)), ValueError),
        (dict(bias=z(5)), ValueError), (dict(bias=z(4, dtype=torch.float16)), ValueError),
        (dict(count=None), ValueError), (dict(seg_ptr=z(4, dtype=torch.int64)), ValueError),
        (dict(count=None, seg_ptr=z(3, dtype=torch.int64)), ValueError), (dict(size=-1), ValueError),
        (dict(gather_indices=z(6)), ValueError), (dict(count=0), ValueError), (dict(count=3), ValueError),
    ]


@pytest.mark.parametrize("i", range(18))
def test_python_side_errors(i):
    import torch
    from euler_amd import ops
    change, error = _bad()[i]
    kw = dict(op="max", table=torch.zeros(6, 8), weight=torch.zeros(8, 4), gather_indices=torch.zeros(6, dtype=torch.int64),
              size=3, bias=torch.zeros(4), count=2)
    kw.update(change)
    with pytest.raises(error):
        ops.pool_aggregate(kw.pop("op"), kw.pop("table"), kw.pop("weight"), kw.pop("gather_indices"), kw.pop("size"), **kw)


if __name__ == "__main__":
    _answer_all()
