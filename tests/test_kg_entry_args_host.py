"""The argument ladder of the six triple-scoring entries (triple_score, triple_score_proj,
triple_score_matrix and their `_grad` forms), driven through the C ABI without a GPU: return code
and the full last-error text of every call that breaks one rule.

The ladder is host arithmetic in front of the first HIP call (CheckKgCall, kg_entry.h, and the tail
of each entry), and libeuler_gpu.so loads without a device, so the pointers here are made-up
addresses that nothing dereferences.  EVERY row stops inside the ladder, in an entry's tail or at
the empty-shape early-out; none may reach a launch.  The calls are made in one child process that
sees no GPU, so that a row which a later change lets through ends in a HIP error (rc -3, a failed
row) and not in a kernel reading address 0x10000 on a device.  The mechanism is that of
test_mp_entry_args_host.py.

A row: (entries, changes to the base call, rc, text); the last error is "<entry>: <text>".  The
base call is valid: 8 triples with 2 negatives, corrupt "both", d 12 (matrix: de 12, dr 8), a 10-row
entity table and 4 relations, fp32, proj 1 with its hyper table, 4 segments, every pointer set
except those proj 1 takes none of.  TRANSFER turns the base into a valid proj 2 call.  The texts
are the answers of the library before the six entries shared one ladder: with that library in
EULER_GPU_LIB_PATH this file passes unchanged."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PTRS = ["ent", "ent_aux_t", "rel", "rel_aux", "matrix", "src", "rel_id", "dst", "neg", "order", "seg_ptr", "seg_rel",
         "pos_out", "neg_out", "g_pos", "g_neg", "g_src", "g_rel", "g_dst", "g_neg_rows", "g_rel_aux", "g_src_aux_t",
         "g_dst_aux_t", "g_neg_aux_rows_t", "gz_src", "gz_dst", "gz_neg_rows", "g_matrix"]
A = {name: 0x10000 * (i + 1) for i, name in enumerate(_PTRS)}          # every address starts on 16 bytes
BASE = dict({n: A[n] for n in _PTRS if not n.endswith("_t")},
            kind=0, normalize=1, corrupt=2, proj=1, ent_aux=None, g_src_aux=None, g_dst_aux=None, g_neg_aux_rows=None,
            ent_dtype=0, rel_dtype=0, matrix_dtype=0, ent_rows=10, rel_rows=4, b=8, k=2, d=12, de=12, dr=8, nseg=4)
TRANSFER = dict(proj=2, ent_aux=A["ent_aux_t"], g_src_aux=A["g_src_aux_t"], g_dst_aux=A["g_dst_aux_t"],
                g_neg_aux_rows=A["g_neg_aux_rows_t"])

_IDS = ["src", "rel_id", "dst", "neg", "b", "k"]
_OUT = ["pos_out", "neg_out"]
_GRAD = ["g_pos", "g_neg", "g_src", "g_rel", "g_dst", "g_neg_rows"]
_S = ["kind", "normalize", "corrupt", "ent", "ent_dtype", "ent_rows", "rel", "rel_dtype", "rel_rows"] + _IDS + ["d"]
_P = ["proj", "kind", "corrupt", "ent", "ent_aux", "ent_dtype", "ent_rows", "rel", "rel_aux", "rel_dtype",
      "rel_rows"] + _IDS + ["d"]
_M = ["kind", "corrupt", "ent", "ent_dtype", "ent_rows", "de", "rel", "rel_dtype", "rel_rows", "dr", "matrix",
      "matrix_dtype"] + _IDS + ["order"]
ARGS = {
    "triple_score": _S + _OUT,
    "triple_score_grad": _S + _GRAD,
    "triple_score_proj": _P + _OUT,
    "triple_score_proj_grad": _P + _GRAD + ["g_rel_aux", "g_src_aux", "g_dst_aux", "g_neg_aux_rows"],
    "triple_score_matrix": _M + _OUT,
    "triple_score_matrix_grad": _M + ["seg_ptr", "seg_rel", "nseg"] + _GRAD + ["gz_src", "gz_dst", "gz_neg_rows",
                                                                             "g_matrix"],
}

SCORE = ("triple_score", "triple_score_grad")
PROJ = ("triple_score_proj", "triple_score_proj_grad")
MATRIX = ("triple_score_matrix", "triple_score_matrix_grad")
ONE_D = SCORE + PROJ                                                    # the entries with one dimension d
ALL = ONE_D + MATRIX
FWD, GRADS = ALL[0::2], ALL[1::2]
PG, MG = PROJ[1:], MATRIX[1:]

E31 = 1 << 31
NOTHING = {n: None for n in _PTRS + ["ent_aux", "g_src_aux", "g_dst_aux", "g_neg_aux_rows"] if not n.endswith("_t")}

T_PROJ = "proj outside 1..2 (1 hyperplane, 2 transfer)"
T_KIND3 = "kind outside 0..2"
T_KIND2 = "kind outside 0..1 (distmult takes no projection)"
T_CORRUPT = "corrupt outside 0..2"
T_DTYPE = "unknown dtype (0 fp32, 1 bf16, 2 fp16)"
T_NEG1 = "b, k or d < 0"
T_NEG2 = "b, k, de or dr < 0"
T_ROWS = "a table with fewer than 1 row"
T_PRODUCT = "b * max(k, 1) * 2 >= 2^31"
T_NULL = "null buffer"
T_AUX = "a missing aux table (proj 1: hyper; proj 2: ent_transfer and rel_transfer)"
T_NONEG = "k > 0 without negatives"
T_ALIGN = "a table is not aligned to its type"
T_OUT = "null output buffer"
T_GNULL = "null gradient buffer"
T_P1 = "proj 1 takes no entity aux gradient buffers"
T_P2 = "proj 2 without its entity aux gradient buffers"
T_NSEG = "nseg outside 0 .. 2^31 - 1"
T_SEG = "nseg > 0 without seg_ptr, seg_rel or g_matrix"
T_GALIGN = "a gradient buffer is not aligned to its type"

ROWS = [
    # ---- the shared ladder, in its order -------------------------------------------------------
    (PROJ, dict(proj=0), -1, T_PROJ),
    (PROJ, dict(proj=3), -1, T_PROJ),
    (SCORE, dict(kind=-1), -1, T_KIND3),
    (SCORE, dict(kind=3), -1, T_KIND3),
    (PROJ + MATRIX, dict(kind=-1), -1, T_KIND2),
    (PROJ + MATRIX, dict(kind=2), -1, T_KIND2),
    (ALL, dict(corrupt=-1), -1, T_CORRUPT),
    (ALL, dict(corrupt=3), -1, T_CORRUPT),
    (ALL, dict(ent_dtype=3), -1, T_DTYPE),
    (ALL, dict(ent_dtype=-1), -1, T_DTYPE),
    (ALL, dict(rel_dtype=3), -1, T_DTYPE),
    (ALL, dict(rel_dtype=-1), -1, T_DTYPE),
    (MATRIX, dict(matrix_dtype=3), -1, T_DTYPE),
    (MATRIX, dict(matrix_dtype=-1), -1, T_DTYPE),
    (ONE_D, dict(b=-1), -1, T_NEG1),
    (ONE_D, dict(k=-1), -1, T_NEG1),
    (ONE_D, dict(d=-1), -1, T_NEG1),
    (MATRIX, dict(b=-1), -1, T_NEG2),
    (MATRIX, dict(k=-1), -1, T_NEG2),
    (MATRIX, dict(de=-1), -1, T_NEG2),
    (MATRIX, dict(dr=-1), -1, T_NEG2),
    (ALL, dict(ent_rows=0), -1, T_ROWS),
    (ALL, dict(rel_rows=0), -1, T_ROWS),
    (ONE_D, dict(d=E31), -1, "d >= 2^31"),
    (MATRIX, dict(de=513), -1, "de or dr above 512"),
    (MATRIX, dict(dr=513), -1, "de or dr above 512"),
    (MATRIX, dict(ent_rows=E31), -1, "ent_rows >= 2^31"),
    (ALL, dict(b=1 << 30), -1, T_PRODUCT),
    (ALL, dict(b=1 << 30, k=0), -1, T_PRODUCT),
    (ALL, dict(b=1 << 20, k=1 << 10), -1, T_PRODUCT),
    (ALL, dict(b=E31, k=0), -1, T_PRODUCT),
    (ALL, dict(b=1, k=E31), -1, T_PRODUCT),
    (PROJ, dict(ent_aux=A["ent_aux_t"]), -1, "proj 1 takes no ent_aux table"),
    # ---- nothing to do: OK before any pointer is looked at --------------------------------------
    (ALL, dict(b=0), 0, None),
    (ONE_D, dict(d=0), 0, None),
    (MATRIX, dict(de=0), 0, None),
    (MATRIX, dict(dr=0), 0, None),
    (ALL, dict(NOTHING, b=0), 0, None),
    (ONE_D, dict(NOTHING, d=0), 0, None),
    (MATRIX, dict(NOTHING, de=0), 0, None),
    (MATRIX, dict(NOTHING, dr=0), 0, None),
    (PROJ, dict(TRANSFER, b=0), 0, None),
    (MG, dict(b=0, nseg=0), 0, None),
    # ---- the pointers of the shared ladder ------------------------------------------------------
    (ALL, dict(ent=None), -1, T_NULL),
    (ALL, dict(rel=None), -1, T_NULL),
    (ALL, dict(src=None), -1, T_NULL),
    (ALL, dict(rel_id=None), -1, T_NULL),
    (ALL, dict(dst=None), -1, T_NULL),
    (MATRIX, dict(matrix=None), -1, T_NULL),
    (MATRIX, dict(order=None), -1, T_NULL),
    (PROJ, dict(rel_aux=None), -1, T_AUX),
    (PROJ, dict(TRANSFER, rel_aux=None), -1, T_AUX),
    (PROJ, dict(TRANSFER, ent_aux=None), -1, T_AUX),
    (ALL, dict(neg=None), -1, T_NONEG),
    (ALL, dict(ent=A["ent"] + 2), -1, T_ALIGN),
    (ALL, dict(rel=A["rel"] + 2), -1, T_ALIGN),
    (ALL, dict(ent_dtype=1, ent=A["ent"] + 1), -1, T_ALIGN),
    (ALL, dict(rel_dtype=2, rel=A["rel"] + 1), -1, T_ALIGN),
    (PROJ, dict(rel_aux=A["rel_aux"] + 2), -1, T_ALIGN),
    (PROJ, dict(rel_dtype=1, rel_aux=A["rel_aux"] + 1), -1, T_ALIGN),
    (PROJ, dict(TRANSFER, ent_aux=A["ent_aux_t"] + 2), -1, T_ALIGN),
    (PROJ, dict(TRANSFER, ent_dtype=2, ent_aux=A["ent_aux_t"] + 1), -1, T_ALIGN),
    (MATRIX, dict(matrix=A["matrix"] + 2), -1, T_ALIGN),
    (MATRIX, dict(matrix_dtype=1, matrix=A["matrix"] + 1), -1, T_ALIGN),
    # ---- the entries' tails ----------------------------------------------------------------------
    (FWD, dict(pos_out=None), -1, T_OUT),
    (FWD, dict(neg_out=None), -1, T_OUT),
    (GRADS, dict(g_pos=None), -1, T_GNULL),
    (GRADS, dict(g_neg=None), -1, T_GNULL),
    (GRADS, dict(g_src=None), -1, T_GNULL),
    (GRADS, dict(g_rel=None), -1, T_GNULL),
    (GRADS, dict(g_dst=None), -1, T_GNULL),
    (GRADS, dict(g_neg_rows=None), -1, T_GNULL),
    (PG, dict(g_rel_aux=None), -1, T_GNULL),
    (MG, dict(gz_src=None), -1, T_GNULL),
    (MG, dict(gz_dst=None), -1, T_GNULL),
    (MG, dict(gz_neg_rows=None), -1, T_GNULL),
    (PG, dict(g_src_aux=A["g_src_aux_t"]), -1, T_P1),
    (PG, dict(g_dst_aux=A["g_dst_aux_t"]), -1, T_P1),
    (PG, dict(g_neg_aux_rows=A["g_neg_aux_rows_t"]), -1, T_P1),
    (PG, dict(TRANSFER, g_src_aux=None), -1, T_P2),
    (PG, dict(TRANSFER, g_dst_aux=None), -1, T_P2),
    (PG, dict(TRANSFER, g_neg_aux_rows=None), -1, T_P2),
    (MG, dict(nseg=-1), -1, T_NSEG),
    (MG, dict(nseg=E31), -1, T_NSEG),
    (MG, dict(seg_ptr=None), -1, T_SEG),
    (MG, dict(seg_rel=None), -1, T_SEG),
    (MG, dict(g_matrix=None), -1, T_SEG),
    (GRADS, dict(g_src=A["g_src"] + 2), -1, T_GALIGN),
    (GRADS, dict(g_rel=A["g_rel"] + 2), -1, T_GALIGN),
    (GRADS, dict(g_dst=A["g_dst"] + 2), -1, T_GALIGN),
    (GRADS, dict(g_neg_rows=A["g_neg_rows"] + 2), -1, T_GALIGN),
    (PG, dict(g_rel_aux=A["g_rel_aux"] + 2), -1, T_GALIGN),
    (PG, dict(TRANSFER, g_src_aux=A["g_src_aux_t"] + 2), -1, T_GALIGN),
    (PG, dict(TRANSFER, g_dst_aux=A["g_dst_aux_t"] + 2), -1, T_GALIGN),
    (PG, dict(TRANSFER, g_neg_aux_rows=A["g_neg_aux_rows_t"] + 2), -1, T_GALIGN),
    (MG, dict(gz_src=A["gz_src"] + 2), -1, T_GALIGN),
    (MG, dict(gz_dst=A["gz_dst"] + 2), -1, T_GALIGN),
    (MG, dict(gz_neg_rows=A["gz_neg_rows"] + 2), -1, T_GALIGN),
    (MG, dict(g_matrix=A["g_matrix"] + 2), -1, T_GALIGN),
    (MG, dict(matrix_dtype=1, g_matrix=A["g_matrix"] + 1), -1, T_GALIGN),
    # ---- which rule answers where two could --------------------------------------------------------
    (PROJ, dict(proj=0, kind=5), -1, T_PROJ),
    (ALL, dict(kind=5, corrupt=5), -1, None),                            # the family's kind text, filled in below
    (ALL, dict(ent_dtype=7, b=-1), -1, T_DTYPE),
    (ALL, dict(ent_rows=0, b=1 << 30), -1, T_ROWS),
    (ALL, dict(b=0, ent_rows=0), -1, T_ROWS),
    (ALL, dict(ent=None, neg=None), -1, T_NULL),
    (ALL, dict(neg=None, ent=A["ent"] + 2), -1, T_NONEG),
    (PROJ, dict(b=0, ent_aux=A["ent_aux_t"]), -1, "proj 1 takes no ent_aux table"),
    (PG, dict(b=0, g_src_aux=A["g_src_aux_t"]), -1, T_P1),
    (PG, dict(kind=5, g_src_aux=A["g_src_aux_t"]), -1, T_KIND2),
    (PG, dict(ent=None, g_src_aux=A["g_src_aux_t"]), -1, T_NULL),
    (MG, dict(b=0, nseg=-1), -1, T_NSEG),
    (MG, dict(kind=5, nseg=-1), -1, T_KIND2),
    (MG, dict(ent=None, nseg=-1), -1, T_NULL),
    (MG, dict(g_pos=None, seg_ptr=None), -1, T_GNULL),
    (FWD, dict(ent=A["ent"] + 2, pos_out=None), -1, T_ALIGN),
]


def _text(row, entry):
    if row[3] is None and row[2] != 0:
        return T_KIND3 if entry in SCORE else T_KIND2
    return row[3]


def _cases(row):
    """the calls of a row: (entry, its argument values in ABI order)"""
    v = dict(BASE, **row[1])
    return [(entry, [v[n] for n in ARGS[entry]]) for entry in row[0]]


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
    assert sorted(ARGS) == sorted({e for row in ROWS for e in row[0]}) and len(ARGS) == 6
    from euler_amd import _lib
    for entry, names in ARGS.items():
        assert len(_lib.SIGNATURES["euler_gpu_" + entry][1]) == 1 + len(names), entry
        assert all(n in BASE for n in names), entry


@pytest.mark.parametrize("i", range(len(ROWS)), ids=lambda i: "%03d-%s" % (i, ROWS[i][0][0]))
def test_row(answers, i):
    row = ROWS[i]
    for (entry, values), (rc, text) in zip(_cases(row), answers[i]):
        assert rc == row[2], (entry, values, rc, text)
        if row[2] != 0:
            assert text == entry + ": " + _text(row, entry), (entry, values)


if __name__ == "__main__":
    _answer_all()
