#!/usr/bin/env python3
"""The auction decoder on the device (tools/assign_bench.py), on noisy-copy embeddings (dim 75, cut 100, eps 1e-3, default floor):
  1. the candidate lists (mke_stable_lists through candidate_lists): host clock around a synchronised call;
  2. the auction to its fixed point (base.alignment._auction: the loop of assignment_matching, its read-backs included) in its
     default form, without the tail kernel (MKE_ASSIGN_NO_TAIL) and over a sweep of tail_cap — host clock, the loop ends in a
     read-back; median of --reps runs after one warm-up run; rounds, bids and the kernel launches each form enqueues;
  3. stable_matching on the same lists, the sibling decoder;
  4. precision of the greedy argmax, the stable matching and the assignment against the gold column = row index;
  5. at --dense-n (a size the CPU can hold as a matrix): scipy.optimize.linear_sum_assignment on the dense float64 matrix — its
     time and optimum — beside the auction's total on the truncated lists.
One JSON line per size and one for the dense comparison.

    python tools/assign_bench.py [--sizes 20000,100000] [--dense-n 5000] [--reps 3] [--caps 1,4,8,16,32,64,256,1024,4096]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def noisy_copy(n, dim, noise, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    e1 = torch.randn(n, dim, device="cuda", generator=g)
    e1 = e1 / e1.norm(dim=1, keepdim=True)
    return e1, e1 + noise * torch.randn(n, dim, device="cuda", generator=g)


def clocked(fn, reps):
    """(median seconds, last result) of a function that ends synchronised; one warm-up run first."""
    fn()
    torch.cuda.synchronize()
    times, out = [], None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    times.sort()
    return times[len(times) // 2], out


def lists_and_floor(e1, e2, cut, reps):
    from multike_amd.base import alignment as AL
    a, b, kpad, code, sq1, sq2 = AL.prepare_operands(e1, e2, "inner", True, "cuda")
    secs, (val, col, redone) = clocked(lambda: AL.candidate_lists(a, b, kpad, cut, code, sq1, sq2), reps)
    listed = (col >= 0) & torch.isfinite(val)
    floor = float(torch.where(listed, val, torch.full_like(val, float("inf"))).min()) - 1.0
    return val, col, floor, secs, redone


def precision(match, n):
    m = match.long()
    matched = int((m >= 0).sum())
    return (int((m == torch.arange(n, device=m.device)).sum()) / matched * 100 if matched else 0.0), matched


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,100000")
    ap.add_argument("--dense-n", type=int, default=5000)
    ap.add_argument("--dim", type=int, default=75)
    ap.add_argument("--cut", type=int, default=100)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--noise", type=float, default=0.18)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--caps", default="1,4,8,16,32,64,256,1024,4096")
    a = ap.parse_args()
    from multike_amd import _lib
    from multike_amd.base import alignment as AL
    assert torch.cuda.is_available(), "assign_bench.py measures on the GPU; there is no CPU path"
    caps = [int(x) for x in a.caps.split(",")]

    def auction(val, col, n, floor, cap, flags):
        return AL._auction(val, col, n, a.eps, floor, AL.ASSIGN_ROUND_BATCH, 1 << 20, cap, flags)

    for n in (int(x) for x in a.sizes.split(",") if x):
        e1, e2 = noisy_copy(n, a.dim, a.noise, n)
        val, col, floor, lists_s, redone = lists_and_floor(e1, e2, a.cut, a.reps)
        res = {"n": n, "dim": a.dim, "cut": a.cut, "eps": a.eps, "floor": round(floor, 4), "lists_s": lists_s, "rows_redone": redone,
               "greedy_precision": float((col[:, 0] == torch.arange(n, device="cuda")).float().mean()) * 100}
        secs, (state, price, progress, launches) = clocked(lambda: auction(val, col, n, floor, 0, 0), a.reps)
        rounds, _, bids, settled = progress.tolist()
        res.update(auction_s=secs, rounds=rounds, bids=bids, settled=settled, launches=launches, default_tail_cap=_lib.ASSIGN_TAIL_CAP)
        res["assign_precision"], res["assign_matched"] = precision(state - 1, n)
        secs, (state2, price2, progress2, launches2) = clocked(lambda: auction(val, col, n, floor, 0, _lib.ASSIGN_NO_TAIL), a.reps)
        res.update(no_tail_s=secs, no_tail_launches=launches2,
                   no_tail_identical=bool(torch.equal(state, state2) and torch.equal(price, price2) and torch.equal(progress, progress2)))
        for cap in caps:
            secs, (s3, p3, g3, l3) = clocked(lambda: auction(val, col, n, floor, cap, 0), a.reps)
            res[f"cap{cap}_s"], res[f"cap{cap}_launches"] = secs, l3
            assert torch.equal(s3, state) and torch.equal(p3, price) and torch.equal(g3, progress), cap
        secs, (match, matched, gold, stable_rounds) = clocked(lambda: AL.stable_matching(val, col, n), a.reps)
        res.update(stable_s=secs, stable_rounds=stable_rounds, stable_precision=gold / matched * 100 if matched else 0.0, stable_matched=matched)
        print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
        del val, col, e1, e2

    n = a.dense_n
    if n > 0:
        from scipy.optimize import linear_sum_assignment
        e1, e2 = noisy_copy(n, a.dim, a.noise, n)
        val, col, floor, _, _ = lists_and_floor(e1, e2, a.cut, 1)
        secs, (state, price, progress, _) = clocked(lambda: auction(val, col, n, floor, 0, 0), a.reps)
        u1, u2 = (x.double() / x.double().norm(dim=1, keepdim=True) for x in (e1, e2))
        dense = (u1 @ u2.T).cpu().numpy()
        t = time.perf_counter()
        r, c = linear_sum_assignment(dense, maximize=True)
        scipy_s = time.perf_counter() - t
        held = state.long() - 1
        rows = torch.nonzero(held >= 0).flatten()
        total = float(torch.as_tensor(dense, device="cuda")[rows, held[rows]].sum()) + floor * int((held < 0).sum())
        res = {"dense_n": n, "cut": a.cut, "eps": a.eps, "auction_s": secs, "rounds": int(progress[0]), "bids": int(progress[2]),
               "auction_total": total, "scipy_s": scipy_s, "scipy_optimum": float(dense[r, c].sum()),
               "gap": float(dense[r, c].sum()) - total, "bound_n_eps": n * (a.eps + 2.0 ** -16),
               "same_pairs": int((torch.as_tensor(c, device="cuda") == held).sum()),
               "assign_precision": precision(held, n)[0], "scipy_precision": float((c == np.arange(n)).mean()) * 100}
        print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
