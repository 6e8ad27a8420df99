#!/usr/bin/env python3
"""Plain vs CSLS alignment evaluation on the device (tools/csls_bench.py): HIP-event times of alignment_counts without and
with CSLS re-scoring (k = 10), and of its parts (r_T + r_S top-k means, the CSLS rank sweep), at n1 = n2 = 10,500 (the
DBP-WD 70 % test split) and 60,000, d = 75; peak torch.cuda allocation of each.  One JSON line per size.

    python tools/csls_bench.py [--sizes 10500,60000] [--k 10] [--reps 5]
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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--dim", type=int, default=75)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from multike_amd import _lib
    from multike_amd.base.alignment import alignment_counts, csls_means, prepare_operands
    for n in (int(x) for x in a.sizes.split(",")):
        g = torch.Generator(device="cuda").manual_seed(n)
        e2 = torch.randn(n, a.dim, device="cuda", generator=g)
        e1 = e2 + 0.7 * torch.randn(n, a.dim, device="cuda", generator=g)
        ap_, bp, kpad, code, _, _ = prepare_operands(e1, e2, "inner", True, "cuda")
        r_t, r_s = csls_means(ap_, bp, kpad, code, None, None, a.k)
        rank, ties, best = (torch.zeros(n, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.int64))

        def sweep_plain():
            _lib.align_rank(ap_, bp, kpad, n, n, rank, best, ties)

        def sweep_csls():
            _lib.align_rank_ex(ap_, bp, kpad, rank, ties, best, code, None, None, r_t, r_s)

        res = {"n": n, "d": a.dim, "k": a.k,
               "plain_ms": timed(lambda: alignment_counts(e1, e2, True), a.reps),
               "csls_ms": timed(lambda: alignment_counts(e1, e2, True, csls_k=a.k), a.reps),
               "plain_sweep_ms": timed(sweep_plain, a.reps),
               "csls_sweep_ms": timed(sweep_csls, a.reps),
               "topk_means_ms": timed(lambda: csls_means(ap_, bp, kpad, code, None, None, a.k), a.reps),
               "r_t_ms": timed(lambda: _lib.align_topk_mean(ap_, bp, kpad, a.k, code), a.reps),
               "euclid_csls_ms": timed(lambda: alignment_counts(e1, e2, False, metric="euclidean", csls_k=a.k), a.reps),
               "plain_peak_mib": peak(lambda: alignment_counts(e1, e2, True)),
               "csls_peak_mib": peak(lambda: alignment_counts(e1, e2, True, csls_k=a.k)),
               "matrix_mib": n * n * 4 / 2**20}
        res["csls_over_plain"] = res["csls_ms"] / res["plain_ms"]
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
