#!/usr/bin/env python3
"""Stable (Gale-Shapley) alignment on the device (tools/stable_bench.py): HIP-event times of the candidate-list pass
(mke_stable_lists, cut = 100, with its share of rows redone as whole rows), of the deferred-acceptance rounds (with their
count) and of the whole stable_alignment call, without and with CSLS re-scoring (k = 10), at n1 = n2 = 10,500 and 60,000,
d = 75; peak torch.cuda allocation of the call; and, on the same operands, the plain evaluator sweep (mke_align_rank) and the
CSLS top-k pass (mke_align_topk_mean) the list pass is reported as a multiple of.  One JSON line per (size, csls).

    python tools/stable_bench.py [--sizes 10500,60000] [--cut 100] [--k 10] [--reps 5]
"""
import argparse
import contextlib
import io
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from csls_bench import peak, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10500,60000")
    ap.add_argument("--cut", type=int, default=100)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--dim", type=int, default=75)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--noise", type=float, default=2.0,
                    help="noise on e1 relative to e2's unit-variance coordinates: at 2.0 about half of the golds are a row's best "
                         "column at 60,000 targets, so suitors compete and the rounds have work to do")
    a = ap.parse_args()
    from multike_amd import _lib
    from multike_amd.base.alignment import candidate_lists, csls_means, prepare_operands, stable_alignment, stable_matching
    for n in (int(x) for x in a.sizes.split(",")):
        g = torch.Generator(device="cuda").manual_seed(n)
        e2 = torch.randn(n, a.dim, device="cuda", generator=g)
        e1 = e2 + a.noise * torch.randn(n, a.dim, device="cuda", generator=g)
        ap_, bp, kpad, code, _, _ = prepare_operands(e1, e2, "inner", True, "cuda")
        rank, ties, best = (torch.zeros(n, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.int64))
        plain_sweep = timed(lambda: _lib.align_rank(ap_, bp, kpad, n, n, rank, best, ties), a.reps)
        topk_pass = timed(lambda: _lib.align_topk_mean(ap_, bp, kpad, a.k, code), a.reps)
        for k in (0, a.k):
            csls = csls_means(ap_, bp, kpad, code, None, None, k) if k else None
            val, col, redone = candidate_lists(ap_, bp, kpad, a.cut, code, None, None, csls)
            _, matched, gold, rounds = stable_matching(val, col, n)

            def whole():
                with contextlib.redirect_stdout(io.StringIO()):
                    stable_alignment(e1, e2, "inner", True, k, 1, cut=a.cut)

            res = {"n": n, "d": a.dim, "cut": a.cut, "csls_k": k, "noise": a.noise,
                   "lists_ms": timed(lambda: candidate_lists(ap_, bp, kpad, a.cut, code, None, None, csls), a.reps),
                   "sweep_only_ms": timed(lambda: _lib.stable_lists(ap_, bp, kpad, a.cut, code, None, None,
                                                                    *(csls if csls else (None, None))), a.reps),
                   "rows_redone": redone,
                   "rounds_ms": timed(lambda: stable_matching(val, col, n), a.reps), "rounds": rounds,
                   "matched": matched, "precision": round(gold / max(matched, 1) * 100, 3),
                   "call_ms": timed(whole, a.reps), "call_peak_mib": peak(whole),
                   "lists_temp_mib": _lib.stable_lists_temp_bytes(n, n, kpad, a.cut) / 2**20, "matrix_mib": n * n * 4 / 2**20,
                   "plain_sweep_ms": plain_sweep, "topk_pass_ms": topk_pass}
            res["lists_over_plain_sweep"] = res["lists_ms"] / plain_sweep
            res["lists_over_topk_pass"] = res["lists_ms"] / topk_pass
            print(json.dumps({kk: (round(v, 3) if isinstance(v, float) else v) for kk, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
