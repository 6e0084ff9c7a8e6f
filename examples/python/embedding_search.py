#!/usr/bin/env python3
"""What a user does with a trained embedding table: exact search and full-table evaluation.

1. The flow of the reference's knn/knn.py: the nearest 10 embeddings of the first 25 rows of a
   table, with and without their own row, through ops.table_topk - no index to train, no [Q, N]
   score block, equal scores in row order on every run.  --composed also runs what the op
   replaces - `queries @ table.T` in row chunks that fit, torch.topk per chunk, the chunks merged -
   and asserts the same rows wherever the composition's scores are distinct.
2. A full-table evaluation: TransE l1 ranks of a batch of triples' tails over ALL entities
   (ops.table_rank with q = h + r), then mrr / hit@10 through ops.rank_metric, beside the rank
   among sampled negatives (ops.triple_score) on the same triples - the number the reference's
   metrics report, which flatters the model.

The table is random (seeded): the example shows the calls, not a trained model."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def composed_scores(table, queries, metric, begin, end):
    """[Q, end - begin] scores of one row chunk in plain torch (larger or smaller is better as in the op)"""
    import torch
    x, q = table[begin:end].float(), queries.float()
    if metric == "ip":
        return q @ x.T
    if metric == "cos":
        inv = lambda t: 1.0 / torch.sqrt(torch.clamp((t * t).sum(1), min=1e-12))        # noqa: E731
        return ((q @ x.T) * inv(q)[:, None]) * inv(x)[None, :]
    out = torch.empty((q.shape[0], x.shape[0]), dtype=torch.float32, device=x.device)
    step = max(1, (1 << 28) // (q.shape[0] * x.shape[1]))               # rows whose [Q, rows, d] block stays inside 1 GiB
    for at in range(0, x.shape[0], step):
        e = q[:, None, :] - x[None, at:at + step, :]
        out[:, at:at + step] = (e * e).sum(-1) if metric == "l2" else e.abs().sum(-1)
    return out


def chunk_rows(q, n, budget_bytes=1 << 30):
    """rows a chunk so that its [Q, rows] fp32 score block stays inside the budget"""
    return max(1, min(n, budget_bytes // (4 * max(q, 1))))


def composed_topk(table, queries, k, metric="ip", exclude=None):
    """The composition: chunked scores, torch.topk per chunk, merged -> (scores [Q, k], rows [Q, k]).
    Needs N - 1 >= k.  Equal scores come out in whatever order torch.topk leaves them."""
    import torch
    n, q = table.shape[0], queries.shape[0]
    largest = metric in ("ip", "cos")
    best_s = best_r = None
    step = chunk_rows(q, n)
    for begin in range(0, n, step):
        end = min(n, begin + step)
        s = composed_scores(table, queries, metric, begin, end)
        if exclude is not None:
            inside = (exclude >= begin) & (exclude < end)
            at = torch.nonzero(inside).reshape(-1)
            s[at, exclude[at] - begin] = float("-inf") if largest else float("inf")
        cs, cr = torch.topk(s, min(k, end - begin), dim=1, largest=largest)
        cr = cr + begin
        if best_s is not None:
            cs, cr = torch.cat([best_s, cs], 1), torch.cat([best_r, cr], 1)
            cs, pick = torch.topk(cs, min(k, cs.shape[1]), dim=1, largest=largest)
            cr = torch.gather(cr, 1, pick)
        best_s, best_r = cs, cr
    return best_s, best_r


def composed_rank(table, queries, target, metric="ip", exclude=None):
    """The composition of the full-table rank: chunked scores, a comparison and a sum per chunk"""
    import torch
    n, q = table.shape[0], queries.shape[0]
    largest = metric in ("ip", "cos")
    ar = torch.arange(q, device=table.device)
    st = composed_scores(table[target], queries, metric, 0, q)[ar, ar]  # (a [Q, Q] block for its diagonal)
    rank = torch.zeros(q, dtype=torch.int64, device=table.device)
    step = chunk_rows(q, n)
    for begin in range(0, n, step):
        end = min(n, begin + step)
        s = composed_scores(table, queries, metric, begin, end)
        hit = (s >= st[:, None]) if largest else (s <= st[:, None])
        for ids in (target, exclude):
            if ids is not None:
                at = torch.nonzero((ids >= begin) & (ids < end)).reshape(-1)
                hit[at, ids[at] - begin] = False
        rank += hit.sum(1)
    return rank.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000, help="rows of the embedding table")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--dtype", default="bfloat16", choices=["float32", "bfloat16", "float16"])
    ap.add_argument("--queries", type=int, default=25)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--triples", type=int, default=512)
    ap.add_argument("--negs", type=int, default=64, help="sampled negatives of the reference's metric")
    ap.add_argument("--composed", action="store_true", help="also run matmul + topk and compare the rows")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import torch
    from euler_amd import ops
    if not torch.cuda.is_available():
        sys.exit("embedding_search: needs a GPU")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    n, d = args.rows, args.dim
    table = (torch.randn((n, d), generator=gen, device="cuda") * d ** -0.5).to(getattr(torch, args.dtype))

    # ---- 1. knn.py: the nearest k of the first rows, with and without their own row ----------
    queries = table[:args.queries]
    own = torch.arange(args.queries, device="cuda")
    for metric in ("l2", "ip"):
        with_self = ops.table_topk(table, queries, args.k, metric=metric)
        without = ops.table_topk(table, queries, args.k, metric=metric, exclude=own)
        if metric == "l2":
            assert torch.all(with_self[0][:, 0] == 0)                    # a row is at distance 0 from itself
        assert not torch.any(without[1] == own[:, None])
        print("[knn %s] query 0: with its own row %s" % (metric, with_self[1][0].tolist()))
        print("[knn %s] query 0: without it       %s" % (metric, without[1][0].tolist()))
        if args.composed:
            cs, cr = composed_topk(table, queries, args.k, metric=metric, exclude=own)
            # the composition's scores differ in the last bits; compare rows where ITS scores are distinct
            spread = (cs[:, 1:] - cs[:, :-1]).abs()
            clear = torch.ones_like(cr, dtype=torch.bool)
            tol = 1e-4 * cs.abs().clamp(min=1.0)
            clear[:, 1:] &= spread > tol[:, 1:]
            clear[:, :-1] &= spread > tol[:, :-1]
            assert torch.all(cr[clear] == without[1][clear]), "the op and the composition disagree on distinct scores"
            print("[knn %s] composed matmul + topk: same rows at %d of %d places (the rest: near-equal scores)"
                  % (metric, int((cr == without[1]).sum()), cr.numel()))

    # ---- 2. TransE: tails ranked over all entities, beside the sampled-negative rank ---------
    n_rel, b = 16, args.triples
    rel = (torch.randn((n_rel, d), generator=gen, device="cuda") * d ** -0.5).to(table.dtype)
    h = torch.randint(0, n, (b,), generator=gen, device="cuda")
    r = torch.randint(0, n_rel, (b,), generator=gen, device="cuda")
    # tails the model "knows": t = the entity nearest to h + r for half the batch, random for the rest
    q = table[h].float() + rel[r].float()
    _, nearest = ops.table_topk(table, q, 1, metric="l1", exclude=h)
    t = torch.where(torch.arange(b, device="cuda") % 2 == 0, nearest[:, 0],
                    torch.randint(0, n, (b,), generator=gen, device="cuda"))
    full = ops.table_rank(table, q, t, metric="l1", exclude=h)
    neg = torch.randint(0, n, (b, args.negs), generator=gen, device="cuda")
    pos_s, neg_s = ops.triple_score(table, rel, h, r, t, neg, kind="trans_l1", corrupt="tail", normalize=False)
    sampled = (neg_s >= pos_s[:, None]).sum(1)
    for name, rank in (("all %d entities" % n, full), ("%d sampled negatives" % args.negs, sampled)):
        print("[transe l1] rank among %-22s mrr %.4f  hit@10 %.4f  mr %.1f"
              % (name + ":", float(ops.rank_metric("mrr", rank)), float(ops.rank_metric("hit10", rank)),
                 float(ops.rank_metric("mr", rank))))
    assert torch.all(full[::2] == 0)                     # the nearest entity (h left out in both calls) ranks first
    assert float(ops.rank_metric("mrr", full)) <= float(ops.rank_metric("mrr", sampled)) + 1e-12
    if args.composed:
        same = int((composed_rank(table, q, t, metric="l1", exclude=h) == full).sum())
        print("[transe l1] composed |q - x| sums + count: the same rank for %d of %d triples" % (same, b))
    print("ok")


if __name__ == "__main__":
    main()
