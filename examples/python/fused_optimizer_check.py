"""What the examples check after one step with --fused-optimizer: the optimisers of euler_amd.optim
are lazy, so only rows that the step looked up may move."""
import torch


def moved_only_looked_up_rows(params, before):
    """-> how many rows of the tables differ from `before`; every one of them is named by its
    table's sparse gradient (the fused optimiser's lazy semantics)"""
    moved_rows = 0
    for p, b in zip(params, before):
        moved = (p.detach() != b).any(dim=1)
        named = torch.zeros_like(moved)
        named[p.grad._indices()[0]] = True
        assert not bool((moved & ~named).any()), "a row that was not looked up moved"
        moved_rows += int(moved.sum())
    return moved_rows
