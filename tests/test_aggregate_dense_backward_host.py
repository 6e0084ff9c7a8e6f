"""What ops.aggregate_dense(backward=...) and euler_gpu_aggregate_dense_backward refuse before a device is asked for,
and the slab rule of csrc/mp_dense_backward.h through the host compiler."""
import os
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT

P = 4096                                                              # a pointer that is never followed
# the entry's arguments after the stream: bf16 (code 1), 5 destinations x count 2 over 10 rows, d 12, F 8, combine add
GOOD = dict(op=1, act=0, combine=1, table=P, dtype=1, rows=10, weight=P, bias=P, bias_dtype=0, gather=P, is_ids=0,
            seg_ptr=None, count=2, e=10, d=12, f=8, size=5, root=P, root_weight=P, ds=6, fs=8, has_scale=0, scale=0.0,
            grad=P, grad_dtype=1, a_ws=P, dzn_ws=P, dzs_ws=P, partial_ws=P, partial_floats=104, d_agg=P, d_weight=P,
            d_bias=P, d_root=P, d_root_weight=P)
BAD = [
    (dict(op=0), "op is 1 mean, 2 add"), (dict(dtype=7), "unknown dtype"), (dict(grad_dtype=2), "grad is fp32 or of the table's dtype"),
    (dict(grad=None), "null buffer"), (dict(d=257), "kDenseBwdMaxK"), (dict(f=513, fs=513), "kDenseBwdMaxF"),
    (dict(ds=257), "kDenseBwdMaxK"), (dict(combine=2, fs=513), "kDenseBwdMaxF"), (dict(fs=9), "combine add needs Fs == F"),
    (dict(seg_ptr=P), "exactly one of seg_ptr and count"), (dict(e=11), "count needs e == size * count"),
    (dict(root=None), "root goes with add"), (dict(bias=None), "d_bias without a bias"),
    (dict(combine=0, root=None, root_weight=None, d_root_weight=None), "d_root without a root"),
    (dict(dzn_ws=None), "without its workspace"), (dict(dzs_ws=None), "without its workspace"),
    (dict(a_ws=None), "without its workspace"), (dict(partial_floats=103), "DenseBwdWorkspaceFloats"),
    (dict(a_ws=P + 8), "not aligned"), (dict(grad=P + 1), "not aligned"), (dict(d_agg=P + 2), "not aligned"),
]


@pytest.mark.parametrize("change,message", BAD, ids=["-".join(c) for c, _ in BAD])
def test_entry_refuses(change, message):
    from euler_amd import _lib
    L = _lib.lib()
    assert L.euler_gpu_aggregate_dense_backward(None, *dict(GOOD, **change).values()) == _lib.EINVAL
    assert message in L.euler_gpu_last_error().decode()


def test_entry_is_declared_bound_and_exported():
    from euler_amd import _lib
    name = "euler_gpu_aggregate_dense_backward"
    assert name + "(" in open(os.path.join(ROOT, "include", "euler_gpu.h")).read()
    assert len(_lib.SIGNATURES[name][1]) == len(GOOD) + 1 and hasattr(_lib.lib(), name)
    # nothing wanted, and size 0: accepted, nothing touched
    none = dict(d_agg=None, d_weight=None, d_bias=None, d_root=None, d_root_weight=None)
    assert _lib.lib().euler_gpu_aggregate_dense_backward(None, *dict(GOOD, **none).values()) == _lib.OK
    assert _lib.lib().euler_gpu_aggregate_dense_backward(None, *dict(GOOD, size=0, e=0).values()) == _lib.OK


def test_python_refuses(monkeypatch):
    from euler_amd import ops
    monkeypatch.setattr(ops, "lib", lambda: pytest.fail("the library was touched"))
    Z = torch.zeros
    gi = Z(6, dtype=torch.int32)
    with pytest.raises(ValueError, match="backward is recompute or fused"):
        ops.aggregate_dense("mean", Z(9, 4), Z(4, 8), gi, 3, count=2, backward="nope")
    with pytest.raises(ValueError, match="kDenseBwdMaxK"):
        ops.aggregate_dense("mean", Z(9, 257), Z(257, 8), gi, 3, count=2, backward="fused")
    with pytest.raises(ValueError, match="kDenseBwdMaxF"):
        ops.aggregate_dense("mean", Z(9, 4), Z(4, 513), gi, 3, count=2, backward="fused")
    with pytest.raises(ValueError, match="kDenseBwdMaxK"):
        ops.aggregate_dense("mean", Z(9, 4), Z(4, 8), gi, 3, count=2, root=Z(3, 300), root_weight=Z(300, 8), backward="fused")
    table = object.__new__(ops.Fp8Rows)             # (its constructor asks for device tensors)
    with pytest.raises(ValueError, match='backward="fused"'):
        ops.aggregate_dense("mean", table, Z(4, 8), gi, 3, count=2, backward="fused")


SLABS = """#include <stdio.h>
#include "mp_dense_backward.h"
using namespace euler_gpu;
int main() {
  const long long sizes[] = {1, 1024, 1025, 2048, 2049, 262144, 262145, 270336, 270337, 2147483647LL};
  for (long long s : sizes)
    printf("%lld %lld %lld %lld\\n", s, (long long)DenseBwdSlabRows(s), (long long)DenseBwdSlabs(s),
           (long long)DenseBwdWorkspaceFloats(s, 12, 8, 6, 8));
  return 0;
}
"""


def test_slab_rule_at_its_boundaries(tmp_path):
    """slabs of 1024 destinations up to 256 of them, then 256 slabs of a multiple of 32; the Python mirror agrees"""
    from euler_amd import ops
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    (tmp_path / "slabs.cc").write_text(SLABS)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "euler_amd", "csrc"),
                           str(tmp_path / "slabs.cc"), "-o", str(tmp_path / "slabs")])
    got = [tuple(map(int, line.split())) for line in subprocess.check_output([str(tmp_path / "slabs")]).decode().splitlines()]
    want = [(1, 1024, 1), (1024, 1024, 1), (1025, 1024, 2), (2048, 1024, 2), (2049, 1024, 3), (262144, 1024, 256),
            (262145, 1056, 249), (270336, 1056, 256), (270337, 1088, 249), (2147483647, 8388608, 256)]
    assert [g[:3] for g in got] == want
    for size, rows, slabs, floats in got:
        assert rows % 32 == 0 and slabs <= 256 and (slabs - 1) * rows < size <= slabs * rows
        assert ops._dense_bwd_slabs(size) == slabs and floats == slabs * (12 * 8 + 8)
