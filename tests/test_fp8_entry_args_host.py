"""The argument ladders of the five entries of the quantised row tables (column_absmax,
fp8_quantize_rows, fp8_gather, fp8_gather_segment_reduce, fp8_gather_segment_reduce_ids), driven
through the C ABI without a GPU: return code and the full last-error text of every call that
breaks one rule - as tests/test_mp_entry_args_host.py does for the sixteen segment-reduce entries.

The two reduce entries go through the ONE ladder of those sixteen (CheckMpReduce, mp_kernels.hip)
in its canonical order: codes, mode / heads, negative shape, empty => OK, null buffers, e >= 2^31,
the 2^24 limits of a mean, params_rows < 2^31, alignment.  All of it is host arithmetic in front
of the first HIP call, and libeuler_gpu.so loads without a device, so the pointers are made-up
addresses nothing dereferences; the calls are made in one child process that sees no GPU, so that
a row a later change lets through ends in a HIP error (rc -3) and not in a kernel reading 0x1000.

A row: (entries, changes to the base call, rc, text).  The base call is valid: d 32, 4
destinations, count 2, a 10-row table, mode 0, fp32 out, fp32 weights [8, 1]; 8 rows / indices for
the three others."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Q, S, G, O, W, X, A = 0x1000, 0x2000, 0x3000, 0x5000, 0x6000, 0x7000, 0x8000
BASE = dict(mode=0, q=Q, scale=S, gather=G, seg_ptr=None, out=O, w=W, w_dtype=0, heads=1, d=32, size=4,
            count=2, params_rows=10, out_dtype=0, x=X, dtype=0, n=8, e=8, absmax=A)

ARGS = {
    "column_absmax": ["x", "dtype", "n", "d", "absmax"],
    "fp8_quantize_rows": ["x", "dtype", "n", "d", "scale", "q"],
    "fp8_gather": ["q", "scale", "gather", "e", "d", "params_rows", "out", "out_dtype"],
    "fp8_gather_segment_reduce": ["mode", "q", "scale", "gather", "seg_ptr", "count", "d", "size", "out",
                                  "out_dtype", "w", "w_dtype", "heads"],
    "fp8_gather_segment_reduce_ids": ["mode", "q", "scale", "params_rows", "gather", "seg_ptr", "count", "d",
                                      "size", "out", "out_dtype", "w", "w_dtype", "heads"],
}

AM, QR, GA = ("column_absmax",), ("fp8_quantize_rows",), ("fp8_gather",)
SR, SRI = ("fp8_gather_segment_reduce",), ("fp8_gather_segment_reduce_ids",)
RED = SR + SRI
CODES = " (0 fp32, 1 bf16, 2 fp16)"
E24, E31 = 1 << 24, 1 << 31


def _red(changes, rc, why):
    """a rule of the shared ladder: one row per reduce entry, each named in its message"""
    return [((e,), changes, rc, None if why is None else "%s: %s" % (e, why)) for e in RED]


ROWS = [
    # ---- column_absmax ------------------------------------------------------------------------
    (AM, dict(dtype=3), -1, "column_absmax: unknown dtype 3" + CODES),
    (AM, dict(dtype=-1), -1, "column_absmax: unknown dtype -1" + CODES),
    (AM, dict(n=-1), -1, "column_absmax: bad shape"),
    (AM, dict(d=-1), -1, "column_absmax: bad shape"),
    (AM, dict(n=0), 0, None),
    (AM, dict(d=0), 0, None),
    (AM, dict(n=0, x=None, absmax=None), 0, None),
    (AM, dict(x=None), -1, "column_absmax: null buffer"),
    (AM, dict(absmax=None), -1, "column_absmax: null buffer"),
    (AM, dict(x=X + 2), -1, "column_absmax: a buffer is not aligned to its type"),
    (AM, dict(dtype=1, x=X + 1), -1, "column_absmax: a buffer is not aligned to its type"),
    (AM, dict(absmax=A + 2), -1, "column_absmax: a buffer is not aligned to its type"),
    # ---- fp8_quantize_rows --------------------------------------------------------------------
    (QR, dict(dtype=4), -1, "fp8_quantize_rows: unknown dtype 4" + CODES),
    (QR, dict(dtype=-1), -1, "fp8_quantize_rows: unknown dtype -1" + CODES),
    (QR, dict(n=-1), -1, "fp8_quantize_rows: bad shape"),
    (QR, dict(d=-1), -1, "fp8_quantize_rows: bad shape"),
    (QR, dict(n=0), 0, None),
    (QR, dict(d=0), 0, None),
    (QR, dict(n=0, x=None, q=None, scale=None), 0, None),
    (QR, dict(x=None), -1, "fp8_quantize_rows: null buffer"),
    (QR, dict(scale=None), -1, "fp8_quantize_rows: null buffer"),
    (QR, dict(q=None), -1, "fp8_quantize_rows: null buffer"),
    (QR, dict(x=X + 1), -1, "fp8_quantize_rows: a buffer is not aligned to its type"),
    (QR, dict(dtype=2, x=X + 1), -1, "fp8_quantize_rows: a buffer is not aligned to its type"),
    (QR, dict(scale=S + 2), -1, "fp8_quantize_rows: a buffer is not aligned to its type"),
    # ---- fp8_gather ---------------------------------------------------------------------------
    (GA, dict(out_dtype=3), -1, "fp8_gather: unknown out_dtype 3" + CODES),
    (GA, dict(out_dtype=-1), -1, "fp8_gather: unknown out_dtype -1" + CODES),
    (GA, dict(e=-1), -1, "fp8_gather: bad shape"),
    (GA, dict(d=-1), -1, "fp8_gather: bad shape"),
    (GA, dict(e=0), 0, None),
    (GA, dict(d=0), 0, None),
    (GA, dict(e=0, q=None, out=None), 0, None),
    (GA, dict(q=None), -1, "fp8_gather: null buffer"),
    (GA, dict(scale=None), -1, "fp8_gather: null buffer"),
    (GA, dict(gather=None), -1, "fp8_gather: null buffer"),
    (GA, dict(out=None), -1, "fp8_gather: null buffer"),
    (GA, dict(out=O + 2), -1, "fp8_gather: a buffer is not aligned to its type"),
    (GA, dict(out_dtype=1, out=O + 1), -1, "fp8_gather: a buffer is not aligned to its type"),
    (GA, dict(scale=S + 1), -1, "fp8_gather: a buffer is not aligned to its type"),
]
# ---- fp8_gather_segment_reduce / _ids: the shared ladder, in its order --------------------------
for _changes, _rc, _why in [
    (dict(out_dtype=3), -1, "unknown out_dtype 3" + CODES),
    (dict(out_dtype=-1), -1, "unknown out_dtype -1" + CODES),
    (dict(out_dtype=8), -1, "unknown out_dtype 8" + CODES),
    (dict(w_dtype=3), -1, "unknown w_dtype 3" + CODES),
    (dict(w_dtype=-1), -1, "unknown w_dtype -1" + CODES),
    (dict(w=W + 2), -1, "the weights are not aligned to their type"),
    (dict(w_dtype=1, w=W + 1), -1, "the weights are not aligned to their type"),
    (dict(mode=-1), -1, "mode is 0 add, 1 max, 2 mean"),
    (dict(mode=3), -1, "mode is 0 add, 1 max, 2 mean"),
    (dict(heads=0), -1, "heads < 1"),
    (dict(heads=5), -1, "heads must divide d"),
    (dict(d=-1), -1, "heads must divide d"),
    (dict(d=-1, w=None), -1, "bad shape"),
    (dict(size=-1), -1, "bad shape"),
    (dict(count=-1), -1, "bad shape"),
    (dict(size=0), 0, None),
    (dict(d=0), 0, None),
    (dict(size=0, q=None, scale=None, out=None, gather=None), 0, None),
    (dict(mode=2, count=E24, size=0), 0, None),
    (dict(out=None), -1, "null buffer"),
    (dict(q=None), -1, "null buffer"),
    (dict(scale=None), -1, "null buffer"),
    (dict(size=2, count=1 << 30), -1, "e >= 2^31"),
    (dict(mode=2, count=E24), -1, "mean needs segments shorter than 2^24"),
    (dict(mode=2, count=E24, w=None), -1, "mean needs segments shorter than 2^24"),
    (dict(out=O + 2), -1, "a buffer is not aligned to its type"),
    (dict(out_dtype=2, out=O + 1), -1, "a buffer is not aligned to its type"),
    (dict(scale=S + 2), -1, "a buffer is not aligned to its type"),
    # the order of the ladder: the earlier rule answers
    (dict(out_dtype=5, mode=9, size=-1), -1, "unknown out_dtype 5" + CODES),
    (dict(mode=9, size=-1, out=None), -1, "mode is 0 add, 1 max, 2 mean"),
    (dict(size=-1, out=None), -1, "bad shape"),
    (dict(out=None, mode=2, count=E24), -1, "null buffer"),
    # w NULL: unweighted - w_dtype and heads are not looked at
    (dict(w=None, w_dtype=7, heads=0, d=0), 0, None),
    (dict(w=None, w_dtype=7, heads=0, out=None), -1, "null buffer"),
]:
    ROWS += _red(_changes, _rc, _why)
ROWS += [
    (SRI, dict(gather=None), -1, "fp8_gather_segment_reduce_ids: null buffer"),
    (SRI, dict(params_rows=E31), -1, "fp8_gather_segment_reduce_ids: the table must have fewer than 2^31 rows"),
    (SRI, dict(params_rows=-1), -1, "fp8_gather_segment_reduce_ids: the table must have fewer than 2^31 rows"),
    (SRI, dict(params_rows=E31, mode=2, count=E24), -1,
     "fp8_gather_segment_reduce_ids: mean needs segments shorter than 2^24"),
    (SRI, dict(params_rows=E31, out=O + 1), -1,
     "fp8_gather_segment_reduce_ids: the table must have fewer than 2^31 rows"),
]


def _cases(row):
    out = []
    for entry in row[0]:
        v = dict(BASE)
        v.update(row[1])
        out.append((entry, [v[n] for n in ARGS[entry]]))
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
    assert sorted(ARGS) == sorted({e for row in ROWS for e in row[0]}) and len(ARGS) == 5
    from euler_amd import _lib
    for entry, names in ARGS.items():
        assert len(_lib.SIGNATURES["euler_gpu_" + entry][1]) == 1 + len(names), entry


@pytest.mark.parametrize("i", range(len(ROWS)), ids=lambda i: "%03d-%s" % (i, ROWS[i][0][0]))
def test_row(answers, i):
    row = ROWS[i]
    for (entry, values), (rc, text) in zip(_cases(row), answers[i]):
        assert rc == row[2], (entry, values, rc, text)
        if row[2] != 0:
            assert text == row[3], (entry, values)


if __name__ == "__main__":
    _answer_all()
