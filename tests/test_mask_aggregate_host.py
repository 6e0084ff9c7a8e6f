"""The errors ops.mask_aggregate raises before it touches a device or loads the library, on
CPU tensors (a call that passed them all ends in the no-CPU-path RuntimeError), and the plan of mp_mask.h,
compiled with the host compiler alone, at its boundaries."""
import pytest
import torch

from mask_aggregate_ref import plan, plan_lib

Z = torch.zeros
I64 = torch.int64
BF = torch.bfloat16
BAD = [
    (dict(op="max"), ValueError), (dict(x=Z(140, 8, dtype=torch.float64)), ValueError), (dict(out_dtype=torch.float16), ValueError),
    (dict(mask=Z(6, 2, dtype=torch.int32)), ValueError), (dict(mask=Z(6, 3, dtype=I64)), ValueError),
    (dict(mask=Z(5, 2, dtype=I64)), ValueError), (dict(mask=Z(12, dtype=I64)), ValueError),
    (dict(x=Z(139, 8)), ValueError), (dict(x=Z(140)), ValueError), (dict(x=Z(140, 0)), ValueError), (dict(x=Z(140, 1025)), ValueError),
    (dict(op="gcn"), ValueError), (dict(op="gcn_renorm"), ValueError), (dict(root=Z(6, 8)), ValueError),
    (dict(op="gcn", root=Z(6, 8, dtype=BF)), ValueError), (dict(op="gcn", root=Z(5, 8)), ValueError),
    (dict(n=-1), ValueError), (dict(batch=2 ** 30, n=2, mask=Z(0, 2, dtype=I64)), ValueError),
    (dict(batch=2 ** 25, m=64, n=0, mask=Z(0, 1, dtype=I64)), ValueError),
    # every rule passed: only now is a device asked for
    ({}, RuntimeError), (dict(op="gcn_renorm", root=Z(6, 8)), RuntimeError), (dict(out_dtype=torch.float32), RuntimeError),
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_python_side_errors(i):
    from euler_amd import ops
    change, error = BAD[i]
    kw = dict(op="add", mask=Z(6, 2, dtype=I64), x=Z(140, 8), batch=2, n=3, m=70)
    kw.update(change)
    with pytest.raises(error):
        ops.mask_aggregate(kw.pop("op"), kw.pop("mask"), kw.pop("x"), kw.pop("batch"), kw.pop("n"), kw.pop("m"), **kw)


# (m, d, fp32) -> (NT, column tiles, candidate block, stride, LDS bytes): mp_mask.h
PLANS = [
    # the column tile: NT 1 | 2 | 4 | 8 at d 16 | 17, 32 | 33, 64 | 65; further column tiles from d = 129
    ((4096, 16, 0), (1, 1, 256, 512, 8192)), ((4096, 17, 0), (2, 1, 256, 512, 16384)), ((4096, 33, 0), (4, 1, 256, 512, 32768)),
    ((4096, 65, 0), (8, 1, 256, 512, 65536)), ((4096, 128, 0), (8, 1, 256, 512, 65536)), ((4096, 129, 0), (8, 2, 256, 512, 65536)),
    ((4096, 1024, 0), (8, 8, 256, 512, 65536)),
    # the candidate block: m rounded up to 64, 256 at most (fp32: 64); packed columns where 2 KB is a multiple of 256
    ((0, 8, 0), (1, 1, 64, 144, 2304)), ((64, 128, 0), (8, 1, 64, 144, 18432)), ((65, 128, 0), (8, 1, 128, 256, 32768)),
    ((129, 128, 0), (8, 1, 192, 400, 51200)), ((193, 128, 0), (8, 1, 256, 512, 65536)), ((257, 128, 0), (8, 1, 256, 512, 65536)),
    ((1, 1, 1), (1, 1, 64, 128, 8192)), ((65, 128, 1), (8, 1, 64, 576, 36864)), ((4096, 1024, 1), (8, 8, 64, 576, 36864)),
]


@pytest.mark.parametrize("shape,want", PLANS, ids=["-".join(map(str, s)) for s, _ in PLANS])
def test_plan_boundaries(shape, want):
    assert plan(*shape) == want


def test_plan_lds_budget_and_tiles():
    for f32 in (0, 1):
        for m in (0, 1, 64, 100, 128, 192, 255, 256, 1000, 4096, 1 << 30):
            for d in (1, 16, 100, 128, 129, 500, 1024):
                nt, tiles, kb, stride, lds = plan(m, d, f32)
                assert lds <= 65536 and kb % 64 == 0 and 16 * nt * tiles >= d > 16 * nt * (tiles - 1)
    lib = plan_lib()
    # a workgroup is 2 waves (64 sources) only where 4 would leave the grid short and n spans more than one such tile
    assert [lib.mask_tile(b, n, c) for b, n, c in [(1, 64, 1), (1, 65, 1), (2, 16384, 1), (1, 16384, 2), (256, 65, 1)]] == \
        [128, 64, 128, 128, 128]
