"""What ops.relation_conv(route=...) and euler_gpu_relation_dense refuse before a device is asked for."""
import os

import pytest
import torch

from conftest import ROOT

P = 4096                                                              # a pointer that is never followed
# the entry's arguments after the stream: mean, bf16 (code 1), 5 destinations x count 2 over 10 rows, R 3, F 12, dim 8
GOOD = dict(mode=2, x=P, dtype=1, rows=10, gather=P, is_ids=0, edge_type=P, num_relations=3, weight=P, seg_ptr=None,
            count=2, e=10, f=12, dim=8, size=5, out=P, out_dtype=1)
BAD = [
    (dict(mode=1), "mode is 0 add, 2 mean"), (dict(mode=4), "mode is 0 add, 2 mean"), (dict(dtype=7), "unknown dtype"),
    (dict(out_dtype=2), "out is fp32 or of x's dtype"), (dict(f=257), "kRelDenseMaxF"), (dict(f=0), "kRelDenseMaxF"),
    (dict(dim=257), "kRelDenseMaxDim"), (dict(dim=0), "kRelDenseMaxDim"), (dict(num_relations=65), "kRelDenseMaxR"),
    (dict(num_relations=0), "kRelDenseMaxR"), (dict(seg_ptr=P), "exactly one of seg_ptr and count"),
    (dict(count=0), "exactly one of seg_ptr and count"), (dict(e=11), "count needs e == size * count"),
    (dict(x=None), "null buffer"), (dict(weight=None), "null buffer"), (dict(edge_type=None), "null buffer"),
    (dict(out=None), "null buffer"), (dict(gather=None, rows=9), "fewer rows than the updates read"),
    (dict(out=P + 1), "not aligned"), (dict(out=P + 2, out_dtype=0), "not aligned"),
]


@pytest.mark.parametrize("change,message", BAD, ids=["-".join(c) + str(i) for i, (c, _) in enumerate(BAD)])
def test_entry_refuses(change, message):
    from euler_amd import _lib
    L = _lib.lib()
    assert L.euler_gpu_relation_dense(None, *dict(GOOD, **change).values()) == _lib.EINVAL
    assert message in L.euler_gpu_last_error().decode()


def test_entry_is_declared_bound_and_exported():
    from euler_amd import _lib
    name = "euler_gpu_relation_dense"
    assert name + "(" in open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    assert len(_lib.SIGNATURES[name][1]) == len(GOOD) + 1 and hasattr(_lib.lib(), name)
    assert _lib.lib().euler_gpu_relation_dense(None, *dict(GOOD, size=0, e=0).values()) == _lib.OK


def test_python_refuses(monkeypatch):
    from euler_amd import ops
    monkeypatch.setattr(ops, "lib", lambda: pytest.fail("the library was touched"))
    Z = torch.zeros
    gi = et = Z(6, dtype=torch.int32)

    def conv(f=4, dim=8, r=3, wdt=torch.float32, **kw):
        return ops.relation_conv(Z(9, f), Z(r, dim, f, dtype=wdt), gi, et, 3, **dict(dict(count=2, route="fused"), **kw))

    with pytest.raises(ValueError, match="route is composed or fused"):
        conv(route="nope")
    for kw, message in ((dict(indices=gi, count=None), "not indices"), (dict(aggr="max"), "aggr is add, mean or mean_rel"),
                        (dict(f=257), "kRelDenseMaxF"), (dict(dim=257), "kRelDenseMaxDim"), (dict(r=65), "kRelDenseMaxR"),
                        (dict(wdt=torch.bfloat16), "one dtype")):
        with pytest.raises(ValueError, match=message) as err:
            conv(**kw)
        assert "aggr" in kw or 'pass route="composed"' in str(err.value)
