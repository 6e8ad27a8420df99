#!/usr/bin/env python3
"""Sinkhorn re-scoring on the device (tools/sinkhorn_bench.py): HIP-event times of one half-iteration (mke_align_lse, row
pass and column pass, with and without sub_b, inner and euclidean) against the plain mke_align_rank sweep timed in the same
process, of the whole evaluation with L iterations against plain and against CSLS k = 10, and the peak torch.cuda allocation
of each, at n1 = n2 = 10,500 (the DBP-WD 70 % test split) and 60,000, d = 75.  One JSON line per size.

    python tools/sinkhorn_bench.py [--sizes 10500,60000] [--iters 10] [--tau 0.05] [--reps 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    times.sort()
    return times[len(times) // 2]


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10500,60000")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--tau", type=float, default=0.05)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--dim", type=int, default=75)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from multike_amd import _lib
    from multike_amd.base.alignment import alignment_counts, prepare_operands, sinkhorn_terms, tie_aware_metrics
    sk = (a.iters, a.tau)
    for n in (int(x) for x in a.sizes.split(",")):
        g = torch.Generator(device="cuda").manual_seed(n)
        e2 = torch.randn(n, a.dim, device="cuda", generator=g)
        e1 = e2 + 0.7 * torch.randn(n, a.dim, device="cuda", generator=g)
        ap_, bp, kpad, code, _, _ = prepare_operands(e1, e2, "inner", True, "cuda")
        _, _, _, ecode, sq1, sq2 = prepare_operands(e1, e2, "euclidean", True, "cuda")
        pa = _lib.align_lse(ap_, bp, kpad, a.tau, code)
        out_a, out_b = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        rank, ties, best = (torch.zeros(n, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.int64))
        r_t, r_s = sinkhorn_terms(ap_, bp, kpad, code, None, None, *sk)

        def hits1(**kw):
            gr, ti, _ = alignment_counts(e1, e2, True, **kw)
            return tie_aware_metrics(gr, ti, [1])[0][0] / n * 100

        res = {"n": n, "d": a.dim, "iters": a.iters, "tau": a.tau,
               "plain_sweep_ms": timed(lambda: _lib.align_rank(ap_, bp, kpad, n, n, rank, best, ties), a.reps),
               "lse_row_ms": timed(lambda: _lib.align_lse(ap_, bp, kpad, a.tau, code, out=out_a), a.reps),
               "lse_col_sub_ms": timed(lambda: _lib.align_lse(bp, ap_, kpad, a.tau, code, sub_b=pa, out=out_b), a.reps),
               "lse_euclid_sub_ms": timed(lambda: _lib.align_lse(bp, ap_, kpad, a.tau, ecode, sq2, sq1, pa, out=out_b), a.reps),
               "rescored_sweep_ms": timed(lambda: _lib.align_rank_ex(ap_, bp, kpad, rank, ties, best, code, None, None, r_t, r_s), a.reps),
               "plain_ms": timed(lambda: alignment_counts(e1, e2, True), a.reps),
               "csls_ms": timed(lambda: alignment_counts(e1, e2, True, csls_k=a.k), a.reps),
               "sinkhorn_ms": timed(lambda: alignment_counts(e1, e2, True, sinkhorn=sk), a.reps),
               "plain_peak_mib": peak(lambda: alignment_counts(e1, e2, True)),
               "csls_peak_mib": peak(lambda: alignment_counts(e1, e2, True, csls_k=a.k)),
               "sinkhorn_peak_mib": peak(lambda: alignment_counts(e1, e2, True, sinkhorn=sk)),
               "lse_temp_mib": _lib.align_lse_temp_bytes(n, n, kpad) / 2**20,
               "matrix_mib": n * n * 4 / 2**20,
               "plain_hits1": hits1(), "csls_hits1": hits1(csls_k=a.k), "sinkhorn_hits1": hits1(sinkhorn=sk)}
        res["half_iteration_over_sweep"] = res["lse_col_sub_ms"] / res["plain_sweep_ms"]
        res["sinkhorn_over_plain"] = res["sinkhorn_ms"] / res["plain_ms"]
        res["sinkhorn_over_csls"] = res["sinkhorn_ms"] / res["csls_ms"]
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
