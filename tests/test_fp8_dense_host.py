"""The errors ops.aggregate_dense raises over an Fp8Rows table, and for root_index, before it touches a device or
loads the library: every new rule of its argument ladder, on CPU tensors (a call that passed them all would end in
the no-CPU-path RuntimeError)."""
import pytest
import torch

Z = torch.zeros
BF, I64 = torch.bfloat16, torch.int64
BAD = [
    (dict(root=Z(3, 8)), ValueError),                                   # root and root_index together
    (dict(table=Z(6, 8)), ValueError),                                  # root_index with an ordinary table
    (dict(root_index=Z(4, dtype=I64)), ValueError), (dict(root_index=Z(3)), ValueError),
    (dict(root_index=Z(3, dtype=torch.int16)), ValueError),
    (dict(root_index=None, root=Z(3, 8, dtype=BF)), ValueError), (dict(root_weight=Z(8, 4, dtype=BF)), ValueError),
    (dict(bias=Z(4, dtype=BF)), ValueError), (dict(weight=Z(8, 4, dtype=BF)), ValueError),
    (dict(weight=Z(8, 4, dtype=torch.float64)), TypeError), (dict(out_dtype=BF), TypeError),
    (dict(weight=Z(7, 4)), ValueError), (dict(root_weight=Z(7, 4)), ValueError),
    (dict(q=Z(6, 1025, dtype=torch.uint8), weight=Z(1025, 4), root_weight=Z(1025, 4)), ValueError),
    (dict(combine="fold"), ValueError), (dict(root_scale=2.0), ValueError),
    # every rule passed: only now is a device asked for
    ({}, RuntimeError), (dict(combine="fold", root_weight=None, root_scale=1.5), RuntimeError),
    (dict(root_index=None, root=Z(3, 5), root_weight=Z(5, 4)), RuntimeError),
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_python_side_errors(i):
    from euler_amd import ops
    change, error = BAD[i]
    kw = dict(op="mean", q=Z(6, 8, dtype=torch.uint8), weight=Z(8, 4), gather_indices=Z(6, dtype=I64), size=3,
              root_index=Z(3, dtype=I64), root_weight=Z(8, 4), bias=Z(4), count=2)
    kw.update(change)
    table = kw.pop("table", None)
    q = kw.pop("q")
    if table is None:               # (the constructor wants device memory: a table of host tensors is put together here)
        table = object.__new__(ops.Fp8Rows)
        table.q, table.scale = q, torch.ones(q.shape[1])
    with pytest.raises(error):
        ops.aggregate_dense(kw.pop("op"), table, kw.pop("weight"), kw.pop("gather_indices"), kw.pop("size"), **kw)
