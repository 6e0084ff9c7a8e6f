"""What ops.pool_aggregate(backward=...) and euler_gpu_pool_aggregate_backward refuse before a device is asked for."""
import os

import pytest
import torch

from conftest import ROOT

P = 4096                                                              # a pointer that is never followed
# the entry's arguments after the stream: max, relu, bf16 (code 1), 5 destinations x count 2 over 10 rows, d 12, F 8
GOOD = dict(op=0, act=0, table=P, dtype=1, rows=10, weight=P, bias=P, bias_dtype=0, gather=P, is_ids=0, seg_ptr=None,
            count=2, e=10, d=12, f=8, size=5, grad=P, grad_dtype=1, dz_ws=P, m_ws=P, share_ws=P, partial_ws=P,
            partial_floats=104, d_rows=P, d_weight=P, d_bias=P)
BAD = [
    (dict(op=3), "op is 0 max, 1 mean, 2 add"), (dict(act=2), "activation is 0 relu, 1 none"), (dict(dtype=7), "unknown dtype"),
    (dict(grad_dtype=2), "grad is fp32 or of the table's dtype"), (dict(grad=None), "null buffer"),
    (dict(d=257), "kPoolBwdMaxK"), (dict(f=513), "kPoolBwdMaxF"), (dict(d=0), "kPoolBwdMaxK"),
    (dict(seg_ptr=P), "exactly one of seg_ptr and count"), (dict(count=0), "exactly one of seg_ptr and count"),
    (dict(e=11), "count needs e == size * count"), (dict(bias=None), "d_bias without a bias"),
    (dict(dz_ws=None), "without its workspace"), (dict(m_ws=None), "without its workspace"),
    (dict(share_ws=None), "without its workspace"), (dict(partial_ws=None), "without its workspace"),
    (dict(partial_floats=103), "PoolBwdWorkspaceFloats"), (dict(dz_ws=P + 8), "not aligned"),
    (dict(grad=P + 1), "not aligned"), (dict(d_rows=P + 2), "not aligned"),
]


@pytest.mark.parametrize("change,message", BAD, ids=["-".join(c) + str(i) for i, (c, _) in enumerate(BAD)])
def test_entry_refuses(change, message):
    from euler_amd import _lib
    L = _lib.lib()
    assert L.euler_gpu_pool_aggregate_backward(None, *dict(GOOD, **change).values()) == _lib.EINVAL
    assert message in L.euler_gpu_last_error().decode()


def test_entry_is_declared_bound_and_exported():
    from euler_amd import _lib
    name = "euler_gpu_pool_aggregate_backward"
    assert name + "(" in open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    assert len(_lib.SIGNATURES[name][1]) == len(GOOD) + 1 and hasattr(_lib.lib(), name)
    # nothing wanted, and size 0: accepted, nothing touched; add needs no m_ws / share_ws to get past the checks
    none = dict(d_rows=None, d_weight=None, d_bias=None)
    assert _lib.lib().euler_gpu_pool_aggregate_backward(None, *dict(GOOD, **none).values()) == _lib.OK
    assert _lib.lib().euler_gpu_pool_aggregate_backward(None, *dict(GOOD, size=0, e=0).values()) == _lib.OK


def test_python_refuses(monkeypatch):
    from euler_amd import ops
    monkeypatch.setattr(ops, "lib", lambda: pytest.fail("the library was touched"))
    Z = torch.zeros
    gi = Z(6, dtype=torch.int32)
    with pytest.raises(ValueError, match="backward is recompute or fused"):
        ops.pool_aggregate("max", Z(9, 4), Z(4, 8), gi, 3, count=2, backward="nope")
    with pytest.raises(ValueError, match="kPoolBwdMaxK"):
        ops.pool_aggregate("max", Z(9, 257), Z(257, 8), gi, 3, count=2, backward="fused")
    with pytest.raises(ValueError, match="kPoolBwdMaxF"):
        ops.pool_aggregate("mean", Z(9, 4), Z(4, 513), gi, 3, count=2, backward="fused")
