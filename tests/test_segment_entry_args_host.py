"""The argument ladders of the ops built on the segment reduces (edge_softmax, segment_attention,
relation_reduce, gather_reduce_norm, gather_segment_topk and their gradients), driven through the
C ABI without a GPU: return code and the full last-error text of every call that breaks one rule,
and of calls that break two adjacent rules of an entry's ladder, which pins the ladder's order - as
tests/test_mp_entry_args_host.py does for the sixteen segment-reduce entries.

Every ladder is host arithmetic in front of the first HIP call, and libeuler_gpu.so loads without
a device, so the pointers here are made-up addresses that nothing dereferences.  EVERY row stops
inside its ladder or at one of its early-outs (`e == 0` for edge_softmax, `size == 0 && e == 0` for
segment_attention, `size == 0 || d == 0` for the others; segment_topk_grad: `e == 0 || d == 0`);
none may reach a launch.  The calls are made in one child process that sees no GPU, so that a row
which a later change lets through ends in a HIP error (rc -3, a failed row) and not in a kernel
reading address 0x1000 on a device.

A row: (entries, changes to the entry's base call, rc, what follows "<name>: " in the message).
Every base call is valid: 8 updates, 4 destinations, count 2, fp32 everywhere, every pointer the
entry needs set, `indices` and `seg_ptr` null.  The table was written against the commit before the
destination resolver (SegDest, mp_segments.h) and passed on its library unchanged: the resolver
moved no rule."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# made-up device addresses, 4096-byte aligned
(A, B, K, S, O, Q, KT, V, G, AL, LG, DS, DQ, T, CN, ND, NS, R, SEL, PE) = [0x1000 * (i + 1) for i in range(20)]

E24, E30, E31 = 1 << 24, 1 << 30, 1 << 31
CODES = " (0 fp32, 1 bf16, 2 fp16)"
FORM = "pass exactly one of indices, seg_ptr and count"
COUNT = "e is not size * count"

_ATT = ["kind", "q", "q_dtype", "q_rows", "q_index", "k", "k_dtype", "k_rows", "v", "v_dtype", "v_rows", "gather",
        "is_ids", "indices", "seg_ptr", "count", "e", "d", "dv", "heads", "size", "scale", "slope"]
_ATT_BASE = dict(kind=0, q=Q, q_dtype=0, q_rows=4, q_index=None, k=KT, k_dtype=0, k_rows=10, v=V, v_dtype=0,
                 v_rows=10, gather=G, is_ids=0, indices=None, seg_ptr=None, count=2, e=8, d=8, dv=8, heads=2,
                 size=4, scale=1.0, slope=0.2)

# entry -> (how its messages begin, argument names in ABI order after the stream, the base call)
ENTRIES = {
    "edge_softmax": (
        "edge_softmax",
        ["a", "in_dtype", "indices", "seg_ptr", "count", "e", "heads", "size", "out", "out_dtype"],
        dict(a=A, in_dtype=0, indices=None, seg_ptr=None, count=2, e=8, heads=1, size=4, out=O, out_dtype=0)),
    "edge_softmax_grad": (
        "edge_softmax_grad",
        ["a", "in_dtype", "b", "b_dtype", "indices", "seg_ptr", "count", "e", "heads", "size", "out", "out_dtype"],
        dict(a=A, in_dtype=0, b=B, b_dtype=0, indices=None, seg_ptr=None, count=2, e=8, heads=1, size=4, out=O,
             out_dtype=0)),
    "segment_attention": (
        "segment_attention", _ATT + ["out", "out_dtype", "alpha", "logits"],
        dict(_ATT_BASE, out=O, out_dtype=0, alpha=None, logits=None)),
    "segment_attention_grad": (
        "segment_attention_grad", _ATT + ["alpha", "grad", "grad_dtype", "ds", "dq_dst"],
        dict(_ATT_BASE, alpha=AL, grad=B, grad_dtype=0, ds=DS, dq_dst=DQ)),
    "relation_reduce": (
        "relation_reduce",
        ["mode", "params", "in_dtype", "rows", "gather", "is_ids", "edge_type", "num_relations", "indices",
         "seg_ptr", "count", "e", "d", "size", "out", "out_dtype", "counts"],
        dict(mode=0, params=A, in_dtype=0, rows=10, gather=G, is_ids=0, edge_type=T, num_relations=3, indices=None,
             seg_ptr=None, count=2, e=8, d=12, size=4, out=O, out_dtype=0, counts=CN)),
    "gather_reduce_norm_t": (
        "gather_reduce_norm",
        ["mode", "params", "in_dtype", "rows", "gather", "indices", "seg_ptr", "count", "e", "d", "size",
         "norm_dst", "norm_src", "root", "root_dtype", "agg_scale", "root_scale", "out", "out_dtype"],
        dict(mode=0, params=A, in_dtype=0, rows=10, gather=G, indices=None, seg_ptr=None, count=2, e=8, d=12,
             size=4, norm_dst=ND, norm_src=NS, root=R, root_dtype=0, agg_scale=1.0, root_scale=1.0, out=O,
             out_dtype=0)),
    "gather_segment_topk": (
        "gather_segment_topk",
        ["params", "in_dtype", "rows", "gather", "is_ids", "seg_ptr", "count", "e", "d", "size", "k", "fill", "out",
         "out_dtype", "sel"],
        dict(params=A, in_dtype=0, rows=10, gather=G, is_ids=0, seg_ptr=None, count=2, e=8, d=12, size=4, k=2,
             fill=0.0, out=O, out_dtype=0, sel=SEL)),
    "segment_topk_grad": (
        "segment_topk_grad", ["grad", "grad_dtype", "sel", "e", "d", "size", "k", "per_edge"],
        dict(grad=B, grad_dtype=0, sel=SEL, e=8, d=12, size=4, k=2, per_edge=PE)),
}

ES, ESG = ("edge_softmax",), ("edge_softmax_grad",)
SMX = ES + ESG
SA, SAG = ("segment_attention",), ("segment_attention_grad",)
ATT = SA + SAG
RR, GN = ("relation_reduce",), ("gather_reduce_norm_t",)
TK, TG = ("gather_segment_topk",), ("segment_topk_grad",)
TOPK = TK + TG

PTR = dict(seg_ptr=S, count=0)                  # the seg_ptr form of a base call
IDX = dict(indices=K, count=0)                  # ... and the indices form
ADDITIVE = dict(kind=1, d=2)                    # segment_attention: additive scores, d == heads
NOT_IN = " is neither fp32 nor the input's dtype"
REL_MEAN = "a mean needs fewer than 2^24 updates (its counts are exact fp32)"
ATT_D = "d is heads (additive) or a multiple of heads (dot)"
TABLE = "a table has no rows, or 2^31 or more"
TK_ALIGN = "a buffer is not aligned to its type"
GN_ALIGN_X = "x, root and out must be aligned to their type"
GN_ALIGN_N = "norm tables and indices must be aligned to their type"

ROWS = [
    # ---- edge_softmax / edge_softmax_grad ------------------------------------------------------
    # ladder: [forward: out_dtype fp32 or in's], dtype codes, heads, negative shape, form, count,
    # e == 0 => OK, null buffers, e >= 2^31
    (SMX, dict(in_dtype=3), -1, "unknown dtype" + CODES),
    (SMX, dict(in_dtype=-1), -1, "unknown dtype" + CODES),
    (ESG, dict(b_dtype=3), -1, "unknown dtype" + CODES),
    (ESG, dict(out_dtype=3), -1, "unknown dtype" + CODES),
    (ESG, dict(out_dtype=-1), -1, "unknown dtype" + CODES),
    (ES, dict(out_dtype=3), -1, "out_dtype is fp32 or in_dtype"),
    (ES, dict(in_dtype=1, out_dtype=2), -1, "out_dtype is fp32 or in_dtype"),
    (ES, dict(in_dtype=0, out_dtype=1), -1, "out_dtype is fp32 or in_dtype"),
    (SMX, dict(heads=0), -1, "heads < 1"),
    (SMX, dict(e=-1), -1, "bad shape"),
    (SMX, dict(size=-1), -1, "bad shape"),
    (SMX, dict(count=-1), -1, "bad shape"),
    (SMX, dict(count=0), -1, FORM),
    (SMX, dict(indices=K), -1, FORM),
    (SMX, dict(seg_ptr=S), -1, FORM),
    (SMX, dict(indices=K, seg_ptr=S, count=0), -1, FORM),
    (SMX, dict(indices=K, seg_ptr=S), -1, FORM),
    (SMX, dict(count=0, e=0), -1, FORM),
    (SMX, dict(count=3), -1, COUNT),
    (SMX, dict(e=9), -1, COUNT),
    (SMX, dict(PTR, e=E31), -1, "e >= 2^31"),
    (SMX, dict(IDX, e=E31), -1, "e >= 2^31"),
    (SMX, dict(a=None), -1, "null buffer"),
    (SMX, dict(out=None), -1, "null buffer"),
    (ESG, dict(b=None), -1, "null buffer"),
    (SMX, dict(PTR, e=0), 0, None),
    (SMX, dict(IDX, e=0), 0, None),
    (SMX, dict(e=0, size=0), 0, None),
    (SMX, dict(PTR, e=0, size=0, a=None, out=None), 0, None),
    # two rules at once, adjacent in the ladder: the first one answers
    (ES, dict(in_dtype=3, out_dtype=1), -1, "unknown dtype" + CODES),
    (ES, dict(out_dtype=1, heads=0), -1, "out_dtype is fp32 or in_dtype"),
    (SMX, dict(in_dtype=3, heads=0), -1, "unknown dtype" + CODES),
    (SMX, dict(heads=0, e=-1), -1, "heads < 1"),
    (SMX, dict(e=-1, indices=K), -1, "bad shape"),
    (SMX, dict(indices=K, count=3), -1, FORM),
    (SMX, dict(count=3, e=0), -1, COUNT),
    (SMX, dict(PTR, e=0, a=None), 0, None),
    (SMX, dict(PTR, e=E31, a=None), -1, "null buffer"),
    (SMX, dict(PTR, e=E31, out=None), -1, "null buffer"),
    (SMX, dict(count=E30, e=E31), -1, COUNT),

    # ---- segment_attention / segment_attention_grad --------------------------------------------
    # ladder: kind, dtype codes, heads, negative shape, d against heads, heads | dv, additive needs v,
    # dv == d without v, form, count, size == 0 && e == 0 => OK, e >= 2^31, null k / gather, table rows,
    # dot needs q, q has rows; then forward: out dtype, null out; grad: grad dtype, null buffers
    (ATT, dict(kind=2), -1, "kind is 0 (dot) or 1 (additive)"),
    (ATT, dict(kind=-1), -1, "kind is 0 (dot) or 1 (additive)"),
    (ATT, dict(k_dtype=3), -1, "unknown dtype" + CODES),
    (ATT, dict(q_dtype=3), -1, "unknown dtype" + CODES),
    (ATT, dict(v_dtype=-1), -1, "unknown dtype" + CODES),
    (ATT, dict(heads=0), -1, "heads < 1"),
    (ATT, dict(e=-1), -1, "bad shape"),
    (ATT, dict(size=-1), -1, "bad shape"),
    (ATT, dict(count=-1), -1, "bad shape"),
    (ATT, dict(d=-2), -1, "bad shape"),
    (ATT, dict(dv=-2), -1, "bad shape"),
    (ATT, dict(d=7), -1, ATT_D),
    (ATT, dict(kind=1), -1, ATT_D),
    (ATT, dict(dv=7), -1, "heads must divide dv"),
    (ATT, dict(ADDITIVE, v=None), -1, "additive attention needs v"),
    (ATT, dict(v=None, dv=4), -1, "without v, dv is d"),
    (ATT, dict(count=0), -1, FORM),
    (ATT, dict(indices=K), -1, FORM),
    (ATT, dict(seg_ptr=S), -1, FORM),
    (ATT, dict(indices=K, seg_ptr=S, count=0), -1, FORM),
    (ATT, dict(indices=K, seg_ptr=S), -1, FORM),
    (ATT, dict(count=3), -1, COUNT),
    (ATT, dict(e=9), -1, COUNT),
    (ATT, dict(PTR, e=E31), -1, "e >= 2^31"),
    (ATT, dict(IDX, e=E31), -1, "e >= 2^31"),
    (ATT, dict(k=None), -1, "null buffer"),
    (ATT, dict(gather=None), -1, "null buffer"),
    (ATT, dict(k_rows=0), -1, TABLE),
    (ATT, dict(v_rows=0), -1, TABLE),
    (ATT, dict(k_rows=E31), -1, TABLE),
    (ATT, dict(v_rows=E31), -1, TABLE),
    (ATT, dict(q=None), -1, "dot attention needs q"),
    (ATT, dict(q_rows=0), -1, "dot attention needs q"),
    (ATT, dict(ADDITIVE, q_rows=0), -1, "q has no rows"),
    (SA, dict(out_dtype=3), -1, "unknown out_dtype"),
    (SA, dict(out_dtype=-1), -1, "unknown out_dtype"),
    (SA, dict(out=None), -1, "null buffer"),
    (SAG, dict(grad_dtype=3), -1, "unknown grad dtype"),
    (SAG, dict(alpha=None), -1, "null buffer"),
    (SAG, dict(ds=None), -1, "null buffer"),
    (SAG, dict(dq_dst=None), -1, "null buffer"),
    (SAG, dict(grad=None), -1, "null buffer"),
    (ATT, dict(e=0, size=0), 0, None),
    (ATT, dict(PTR, e=0, size=0), 0, None),
    (ATT, dict(IDX, e=0, size=0), 0, None),
    (ATT, dict(e=0, size=0, q=None, k=None, v=None, gather=None, dv=8), 0, None),
    (SA, dict(e=0, size=0, out=None, out_dtype=3), 0, None),
    (SAG, dict(e=0, size=0, alpha=None, grad=None, grad_dtype=3, ds=None, dq_dst=None), 0, None),
    # two rules at once
    (ATT, dict(kind=2, k_dtype=3), -1, "kind is 0 (dot) or 1 (additive)"),
    (ATT, dict(k_dtype=3, heads=0), -1, "unknown dtype" + CODES),
    (ATT, dict(heads=0, e=-1), -1, "heads < 1"),
    (ATT, dict(d=-1), -1, "bad shape"),
    (ATT, dict(d=7, dv=7), -1, ATT_D),
    (ATT, dict(ADDITIVE, dv=7, v=None), -1, "heads must divide dv"),
    (ATT, dict(ADDITIVE, v=None, dv=8), -1, "additive attention needs v"),
    (ATT, dict(v=None, dv=4, count=0), -1, "without v, dv is d"),
    (ATT, dict(indices=K, count=3), -1, FORM),
    (ATT, dict(count=0, e=0, size=0), -1, FORM),
    (ATT, dict(count=E30, e=E31), -1, COUNT),
    (ATT, dict(PTR, e=E31, k=None), -1, "e >= 2^31"),
    (ATT, dict(k=None, k_rows=0), -1, "null buffer"),
    (ATT, dict(k_rows=0, q=None), -1, TABLE),
    (SA, dict(ADDITIVE, q_rows=0, out_dtype=3), -1, "q has no rows"),
    (SAG, dict(ADDITIVE, q_rows=0, grad_dtype=3), -1, "q has no rows"),
    (SA, dict(out_dtype=3, out=None), -1, "unknown out_dtype"),
    (SAG, dict(grad_dtype=3, ds=None), -1, "unknown grad dtype"),

    # ---- relation_reduce -----------------------------------------------------------------------
    # ladder: mode, num_relations, negative shape, dtype code, out dtype, form, count, e >= 2^31,
    # size * num_relations, the 2^24 limits of a mean, size == 0 || d == 0 => OK, null out, null
    # params / edge_type, table rows
    (RR, dict(mode=-1), -1, "mode is 0 add, 1 max, 2 mean over the destination, 3 mean over the bucket"),
    (RR, dict(mode=4), -1, "mode is 0 add, 1 max, 2 mean over the destination, 3 mean over the bucket"),
    (RR, dict(num_relations=0), -1, "num_relations < 1"),
    (RR, dict(e=-1), -1, "bad shape"),
    (RR, dict(d=-1), -1, "bad shape"),
    (RR, dict(size=-1), -1, "bad shape"),
    (RR, dict(count=-1), -1, "bad shape"),
    (RR, dict(rows=-1), -1, "bad shape"),
    (RR, dict(in_dtype=3), -1, "unknown dtype" + CODES),
    (RR, dict(in_dtype=-1), -1, "unknown dtype" + CODES),
    (RR, dict(out_dtype=3), -1, "out_dtype is fp32 or in_dtype"),
    (RR, dict(in_dtype=1, out_dtype=2), -1, "out_dtype is fp32 or in_dtype"),
    (RR, dict(in_dtype=0, out_dtype=1), -1, "out_dtype is fp32 or in_dtype"),
    (RR, dict(count=0), -1, FORM),
    (RR, dict(indices=K), -1, FORM),
    (RR, dict(seg_ptr=S), -1, FORM),
    (RR, dict(indices=K, seg_ptr=S, count=0), -1, FORM),
    (RR, dict(indices=K, seg_ptr=S), -1, FORM),
    (RR, dict(count=0, e=0), -1, FORM),
    (RR, dict(count=3), -1, COUNT),
    (RR, dict(e=9), -1, COUNT),
    (RR, dict(PTR, e=E31), -1, "e >= 2^31"),
    (RR, dict(IDX, e=E31), -1, "e >= 2^31"),
    (RR, dict(PTR, size=E30, num_relations=2), -1, "size * num_relations >= 2^31"),
    (RR, dict(PTR, mode=2, e=E24), -1, REL_MEAN),
    (RR, dict(IDX, mode=3, e=E24), -1, REL_MEAN),
    (RR, dict(mode=2, count=E24, size=0, e=0), -1, REL_MEAN),
    (RR, dict(size=0, e=0), 0, None),
    (RR, dict(d=0), 0, None),
    (RR, dict(PTR, size=0), 0, None),
    (RR, dict(d=0, params=None, out=None, edge_type=None, gather=None, counts=None), 0, None),
    (RR, dict(out=None), -1, "null buffer"),
    (RR, dict(params=None), -1, "null buffer"),
    (RR, dict(edge_type=None), -1, "null buffer"),
    (RR, dict(rows=0), -1, "the table has fewer rows than the updates read"),
    (RR, dict(gather=None, rows=7), -1, "the table has fewer rows than the updates read"),
    # two rules at once
    (RR, dict(mode=4, num_relations=0), -1, "mode is 0 add, 1 max, 2 mean over the destination, 3 mean over the bucket"),
    (RR, dict(num_relations=0, e=-1), -1, "num_relations < 1"),
    (RR, dict(d=-1, in_dtype=3), -1, "bad shape"),
    (RR, dict(in_dtype=3, out_dtype=1), -1, "unknown dtype" + CODES),
    (RR, dict(out_dtype=1, count=0), -1, "out_dtype is fp32 or in_dtype"),
    (RR, dict(indices=K, count=3), -1, FORM),
    (RR, dict(count=E30, e=E31), -1, COUNT),
    (RR, dict(PTR, e=E31, size=E30, num_relations=2), -1, "e >= 2^31"),
    (RR, dict(PTR, size=E30, num_relations=2, mode=2, e=E24), -1, "size * num_relations >= 2^31"),
    (RR, dict(PTR, mode=2, e=E24, d=0), -1, REL_MEAN),
    (RR, dict(d=0, out=None), 0, None),
    (RR, dict(out=None, params=None), -1, "null buffer"),
    (RR, dict(params=None, rows=0), -1, "null buffer"),

    # ---- gather_reduce_norm_t ------------------------------------------------------------------
    # ladder: dtype code, out dtype, root dtype, mode, negative shape, form (none allowed when e == 0),
    # count, size == 0 || d == 0 => OK, null buffers, e >= 2^31, rows >= 2^31, the 2^24 limits of a
    # mean, alignment of x / root / out, alignment of the norm tables and indices
    (GN, dict(in_dtype=3), -1, "unknown dtype 3" + CODES),
    (GN, dict(in_dtype=-1), -1, "unknown dtype -1" + CODES),
    (GN, dict(out_dtype=3), -1, "out_dtype 3" + NOT_IN),
    (GN, dict(in_dtype=1, out_dtype=2), -1, "out_dtype 2" + NOT_IN),
    (GN, dict(in_dtype=0, out_dtype=1), -1, "out_dtype 1" + NOT_IN),
    (GN, dict(root_dtype=3), -1, "root_dtype 3" + NOT_IN),
    (GN, dict(in_dtype=1, root_dtype=2), -1, "root_dtype 2" + NOT_IN),
    (GN, dict(mode=1), -1, "max is not supported (mode is 0 add, 2 mean)"),
    (GN, dict(mode=-1), -1, "mode is 0 add, 2 mean"),
    (GN, dict(mode=3), -1, "mode is 0 add, 2 mean"),
    (GN, dict(e=-1), -1, "bad shape"),
    (GN, dict(d=-1), -1, "bad shape"),
    (GN, dict(size=-1), -1, "bad shape"),
    (GN, dict(rows=-1), -1, "bad shape"),
    (GN, dict(count=-1), -1, "bad shape"),
    (GN, dict(count=0), -1, FORM),
    (GN, dict(indices=K), -1, FORM),
    (GN, dict(seg_ptr=S), -1, FORM),
    (GN, dict(indices=K, seg_ptr=S, count=0), -1, FORM),
    (GN, dict(indices=K, seg_ptr=S), -1, FORM),
    (GN, dict(indices=K, seg_ptr=S, count=0, e=0), -1, FORM),
    (GN, dict(count=3), -1, COUNT),
    (GN, dict(e=9), -1, COUNT),
    (GN, dict(size=0, e=0), 0, None),
    (GN, dict(d=0), 0, None),
    (GN, dict(PTR, size=0), 0, None),
    (GN, dict(d=0, params=None, gather=None, norm_dst=None, norm_src=None, root=None, out=None), 0, None),
    # no form at all with e == 0: accepted, so the call ends at the early-out or at a later rule
    (GN, dict(count=0, e=0, size=0), 0, None),
    (GN, dict(count=0, e=0, d=0), 0, None),
    (GN, dict(count=0, e=0, out=None), -1, "null buffer"),
    (GN, dict(out=None), -1, "null buffer"),
    (GN, dict(norm_dst=None), -1, "null buffer"),
    (GN, dict(params=None), -1, "null buffer"),
    (GN, dict(gather=None), -1, "null buffer"),
    (GN, dict(norm_src=None), -1, "null buffer"),
    (GN, dict(PTR, e=E31), -1, "e >= 2^31"),
    (GN, dict(IDX, e=E31), -1, "e >= 2^31"),
    (GN, dict(rows=E31), -1, "the table must have fewer than 2^31 rows"),
    (GN, dict(PTR, mode=2, e=E24), -1, "mean needs e < 2^24"),
    (GN, dict(IDX, mode=2, e=E24), -1, "mean needs e < 2^24"),
    (GN, dict(mode=2, count=E24, size=1, e=E24), -1, "mean needs segments shorter than 2^24"),
    (GN, dict(params=A + 2), -1, GN_ALIGN_X),
    (GN, dict(in_dtype=1, params=A + 1), -1, GN_ALIGN_X),
    (GN, dict(out=O + 2), -1, GN_ALIGN_X),
    (GN, dict(in_dtype=2, out_dtype=2, out=O + 1), -1, GN_ALIGN_X),
    (GN, dict(root=R + 2), -1, GN_ALIGN_X),
    (GN, dict(in_dtype=1, root_dtype=1, root=R + 1), -1, GN_ALIGN_X),
    (GN, dict(norm_dst=ND + 2), -1, GN_ALIGN_N),
    (GN, dict(norm_src=NS + 2), -1, GN_ALIGN_N),
    (GN, dict(gather=G + 2), -1, GN_ALIGN_N),
    (GN, dict(IDX, indices=K + 2), -1, GN_ALIGN_N),
    (GN, dict(PTR, seg_ptr=S + 4), -1, GN_ALIGN_N),
    # two rules at once
    (GN, dict(in_dtype=3, out_dtype=1), -1, "unknown dtype 3" + CODES),
    (GN, dict(out_dtype=1, root_dtype=1), -1, "out_dtype 1" + NOT_IN),
    (GN, dict(root_dtype=1, mode=1), -1, "root_dtype 1" + NOT_IN),
    (GN, dict(mode=1, e=-1), -1, "max is not supported (mode is 0 add, 2 mean)"),
    (GN, dict(mode=3, e=-1), -1, "mode is 0 add, 2 mean"),
    (GN, dict(e=-1, indices=K), -1, "bad shape"),
    (GN, dict(indices=K, count=3), -1, FORM),
    (GN, dict(count=3, d=0), -1, COUNT),
    (GN, dict(d=0, out=None), 0, None),
    (GN, dict(PTR, e=E31, out=None), -1, "null buffer"),
    (GN, dict(PTR, e=E31, rows=E31), -1, "e >= 2^31"),
    (GN, dict(PTR, rows=E31, mode=2, e=E24), -1, "the table must have fewer than 2^31 rows"),
    (GN, dict(mode=2, count=E24, size=1, e=E24, params=A + 2), -1, "mean needs segments shorter than 2^24"),
    (GN, dict(PTR, mode=2, e=E24, params=A + 2), -1, "mean needs e < 2^24"),
    (GN, dict(params=A + 2, norm_dst=ND + 2), -1, GN_ALIGN_X),

    # ---- gather_segment_topk / segment_topk_grad -----------------------------------------------
    # ladder: k, dtype codes, [out dtype], negative shape, 2^31 limits, [form, count], the empty case
    # => OK (size == 0 || d == 0; grad: e == 0 || d == 0), null buffers, [table rows], alignment
    (TOPK, dict(k=0), -1, "k outside 1..16"),
    (TOPK, dict(k=17), -1, "k outside 1..16"),
    (TK, dict(in_dtype=3), -1, "unknown dtype" + CODES),
    (TK, dict(in_dtype=-1), -1, "unknown dtype" + CODES),
    (TK, dict(out_dtype=3), -1, "unknown dtype" + CODES),
    (TG, dict(grad_dtype=3), -1, "unknown dtype" + CODES),
    (TG, dict(grad_dtype=-1), -1, "unknown dtype" + CODES),
    (TK, dict(in_dtype=1, out_dtype=2), -1, "out is fp32 or of the input's dtype"),
    (TK, dict(in_dtype=0, out_dtype=1), -1, "out is fp32 or of the input's dtype"),
    (TK, dict(size=-1), -1, "size, e, d or count < 0"),
    (TK, dict(e=-1), -1, "size, e, d or count < 0"),
    (TK, dict(d=-1), -1, "size, e, d or count < 0"),
    (TK, dict(count=-1), -1, "size, e, d or count < 0"),
    (TG, dict(size=-1), -1, "size, e or d < 0"),
    (TG, dict(e=-1), -1, "size, e or d < 0"),
    (TG, dict(d=-1), -1, "size, e or d < 0"),
    (TOPK, dict(e=E31), -1, "e or d >= 2^31"),
    (TOPK, dict(d=E31), -1, "e or d >= 2^31"),
    (TK, dict(count=0), -1, "exactly one of seg_ptr and count"),
    (TK, dict(seg_ptr=S), -1, "exactly one of seg_ptr and count"),
    (TK, dict(count=3), -1, "count needs e == size * count"),
    (TK, dict(e=9), -1, "count needs e == size * count"),
    (TK, dict(size=0, e=0), 0, None),
    (TK, dict(d=0), 0, None),
    (TK, dict(PTR, size=0), 0, None),
    (TK, dict(d=0, params=None, gather=None, out=None, sel=None), 0, None),
    (TG, dict(e=0), 0, None),
    (TG, dict(d=0), 0, None),
    (TG, dict(e=0, grad=None, sel=None, per_edge=None), 0, None),
    (TK, dict(params=None), -1, "null buffer"),
    (TK, dict(out=None), -1, "null buffer"),
    (TG, dict(per_edge=None), -1, "null buffer"),
    (TG, dict(grad=None), -1, "null buffer"),
    (TG, dict(sel=None), -1, "null buffer"),
    (TG, dict(size=0, per_edge=None), -1, "null buffer"),
    (TK, dict(rows=0), -1, "a table with fewer than 1 row"),
    (TK, dict(rows=-1), -1, "a table with fewer than 1 row"),
    (TK, dict(params=A + 2), -1, TK_ALIGN),
    (TK, dict(in_dtype=1, params=A + 1), -1, TK_ALIGN),
    (TK, dict(out=O + 2), -1, TK_ALIGN),
    (TK, dict(in_dtype=2, out_dtype=2, out=O + 1), -1, TK_ALIGN),
    (TK, dict(sel=SEL + 2), -1, TK_ALIGN),
    (TK, dict(PTR, seg_ptr=S + 4), -1, TK_ALIGN),
    (TK, dict(gather=G + 2), -1, TK_ALIGN),
    (TK, dict(is_ids=1, gather=G + 4), -1, TK_ALIGN),
    (TG, dict(grad=B + 2), -1, TK_ALIGN),
    (TG, dict(grad_dtype=1, grad=B + 1), -1, TK_ALIGN),
    (TG, dict(sel=SEL + 2), -1, TK_ALIGN),
    (TG, dict(per_edge=PE + 2), -1, TK_ALIGN),
    # two rules at once
    (TK, dict(k=0, in_dtype=3), -1, "k outside 1..16"),
    (TG, dict(k=17, grad_dtype=3), -1, "k outside 1..16"),
    (TK, dict(in_dtype=3, out_dtype=1), -1, "unknown dtype" + CODES),
    (TK, dict(out_dtype=1, e=-1), -1, "out is fp32 or of the input's dtype"),
    (TG, dict(grad_dtype=3, e=-1), -1, "unknown dtype" + CODES),
    (TK, dict(size=-1, d=E31), -1, "size, e, d or count < 0"),
    (TG, dict(size=-1, d=E31), -1, "size, e or d < 0"),
    (TK, dict(e=E31, seg_ptr=S), -1, "e or d >= 2^31"),
    (TK, dict(seg_ptr=S, count=3), -1, "exactly one of seg_ptr and count"),
    (TK, dict(count=3, d=0), -1, "count needs e == size * count"),
    (TK, dict(d=0, params=None), 0, None),
    (TK, dict(params=None, rows=0), -1, "null buffer"),
    (TK, dict(rows=0, out=O + 2), -1, "a table with fewer than 1 row"),
    (TG, dict(e=E31, d=0), -1, "e or d >= 2^31"),
    (TG, dict(e=0, per_edge=None), 0, None),
    (TG, dict(grad=None, sel=SEL + 2), -1, "null buffer"),
]


def _cases(row):
    """the calls of a row: (entry, its argument values in ABI order)"""
    out = []
    for entry in row[0]:
        _, names, base = ENTRIES[entry]
        unknown = set(row[1]) - set(names)
        assert not unknown, (entry, unknown)
        v = dict(base, **row[1])
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
    assert sorted(ENTRIES) == sorted({e for row in ROWS for e in row[0]}) and len(ENTRIES) == 8
    from euler_amd import _lib
    for entry, (_, names, base) in ENTRIES.items():
        assert len(_lib.SIGNATURES["euler_gpu_" + entry][1]) == 1 + len(names), entry
        assert sorted(names) == sorted(base), entry


@pytest.mark.parametrize("i", range(len(ROWS)), ids=lambda i: "%03d-%s" % (i, ROWS[i][0][0]))
def test_row(answers, i):
    row = ROWS[i]
    for (entry, values), (rc, text) in zip(_cases(row), answers[i]):
        assert rc == row[2], (entry, values, rc, text)
        if row[2] != 0:
            assert text == "%s: %s" % (ENTRIES[entry][0], row[3]), (entry, values)


if __name__ == "__main__":
    _answer_all()
