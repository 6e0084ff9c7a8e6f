"""The errors ops.mask_attention raises before it touches a device or loads the library, on CPU tensors: a
call that passed them all ends in the no-CPU-path RuntimeError."""
import pytest
import torch

Z = torch.zeros
I64 = torch.int64
BF = torch.bfloat16
# the base call: batch 2, n 3, m 70, 2 heads of 4 columns
BAD = [
    (dict(z=Z(140, 8, dtype=torch.float64)), ValueError), (dict(out_dtype=torch.float16), ValueError),
    (dict(mask=Z(6, 2, dtype=torch.int32)), ValueError), (dict(mask=Z(6, 3, dtype=I64)), ValueError), (dict(mask=Z(12, dtype=I64)), ValueError),
    (dict(z=Z(139, 8)), ValueError), (dict(z=Z(140)), ValueError), (dict(z=Z(140, 0)), ValueError),
    (dict(z=Z(140, 1026), heads=2), ValueError), (dict(heads=0), ValueError), (dict(heads=3), ValueError),
    (dict(s_src=Z(6, 2, dtype=BF)), ValueError), (dict(s_src=Z(5, 2)), ValueError), (dict(s_src=Z(6, 1)), ValueError), (dict(s_src=Z(12)), ValueError),
    (dict(s_nb=Z(139, 2)), ValueError), (dict(s_nb=Z(140, 2, dtype=torch.float64)), ValueError),
    (dict(s_root=Z(6, 2)), ValueError), (dict(root=Z(6, 8), s_root=Z(6, 1)), ValueError), (dict(root=Z(6, 8), s_root=Z(7, 2)), ValueError),
    (dict(root=Z(6, 8, dtype=BF)), ValueError), (dict(root=Z(5, 8)), ValueError),
    (dict(negative_slope=-0.1), ValueError), (dict(negative_slope=float("inf")), ValueError), (dict(negative_slope=float("nan")), ValueError),
    (dict(activation="tanh"), ValueError), (dict(n=-1), ValueError),
    (dict(batch=2 ** 30, n=2, mask=Z(0, 2, dtype=I64)), ValueError),
    # every rule passed: only now is a device asked for
    ({}, RuntimeError), (dict(root=Z(6, 8)), RuntimeError), (dict(root=Z(6, 8), s_root=Z(6, 2), activation="relu"), RuntimeError),
    (dict(s_nb=Z(141, 2), out_dtype=torch.float32, negative_slope=1.0), RuntimeError),
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_python_side_errors(i, monkeypatch):
    from euler_amd import ops
    monkeypatch.setattr(ops, "lib", lambda: pytest.fail("the library was touched"))
    change, error = BAD[i]
    kw = dict(mask=Z(6, 2, dtype=I64), z=Z(140, 8), s_src=Z(6, 2), s_nb=Z(140, 2), batch=2, n=3, m=70, heads=2)
    kw.update(change)
    with pytest.raises(error):
        ops.mask_attention(**kw)
