"""What ops.mask_attention(backward=...) and euler_gpu_mask_attention_backward refuse before a device is asked for."""
import ctypes as C

import pytest
import torch

P = 4096                                                              # a pointer that is never followed
# (mask, mask_t, z, dtype, z rows, s_src, s_nb, s_nb rows, root, s_root, out, grad, grad dtype, batch, n, m, d, heads, slope,
#  activation, stats, d_z, d_s_src, d_s_nb, d_root, d_s_root): batch 2, n 3, m 70, 2 heads of 4 columns, bf16 (code 1)
GOOD = dict(mask=P, mask_t=P, z=P, dtype=1, z_rows=140, s_src=P, s_nb=P, s_nb_rows=140, root=P, s_root=P, out=P, grad=P,
            grad_dtype=1, batch=2, n=3, m=70, d=8, heads=2, slope=0.2, activation=1, stats=P, d_z=P, d_s_src=P, d_s_nb=P,
            d_root=P, d_s_root=P)
BAD = [dict(dtype=7), dict(grad_dtype=2), dict(out=None), dict(root=None, d_root=None), dict(s_root=None), dict(stats=None),
       dict(grad=P + 1), dict(d_z=P + 1), dict(d_s_nb=P + 2), dict(mask_t=None), dict(heads=3), dict(z_rows=139)]


@pytest.mark.parametrize("change", BAD, ids=lambda c: "-".join(c))
def test_entry_refuses(change):
    from euler_amd import _lib
    args = list(dict(GOOD, **change).values())
    assert _lib.lib().euler_gpu_mask_attention_backward(None, *args) == _lib.EINVAL


def test_unknown_backward_is_a_value_error(monkeypatch):
    from euler_amd import ops
    monkeypatch.setattr(ops, "lib", lambda: pytest.fail("the library was touched"))
    Z = torch.zeros
    with pytest.raises(ValueError):
        ops.mask_attention(Z(6, 2, dtype=torch.int64), Z(140, 8), Z(6, 2), Z(140, 2), 2, 3, 70, heads=2, backward="nope")
