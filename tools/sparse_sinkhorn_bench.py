#!/usr/bin/env python3
"""Sparse against dense Sinkhorn re-scoring on the device (tools/sparse_sinkhorn_bench.py): HIP-event times of the dense
potentials (sinkhorn_potentials: 2 * iters sweeps of mke_align_lse) against the sparse ones, whose parts are timed one by one —
the two list sweeps (candidate_lists both ways), the support build (mke_sparse_support), the 2 * iters passes of
mke_sparse_lse — and the Hits@1 of the plain, the dense and the sparse re-scoring, on planted data (e2 = a Gaussian base,
e1 = base + noise * Gaussian, unit rows).  One JSON line per shape.

    python tools/sparse_sinkhorn_bench.py [--shapes 60000x75,100000x256] [--iters 10] [--tau 0.05] [--cut 100] [--reps 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="60000x75,100000x256")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--tau", type=float, default=0.05)
    ap.add_argument("--cut", type=int, default=100)
    ap.add_argument("--noise", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-dense", action="store_true", help="skip the dense path (shapes at which it takes minutes)")
    a = ap.parse_args()
    from multike_amd import _lib
    from multike_amd.base import alignment as al
    for n, d in ((int(x) for x in s.split("x")) for s in a.shapes.split(",")):
        g = torch.Generator(device="cuda").manual_seed(n + d)
        e2 = torch.randn(n, d, device="cuda", generator=g)
        e1 = e2 + a.noise * torch.randn(n, d, device="cuda", generator=g)
        ops = al.prepare_operands(e1, e2, "inner", True, "cuda")
        pa, pb, kpad, code, _, _ = ops
        cut = max(1, min(a.cut, n))
        lists = {}

        def sweep_rows():
            lists["r"] = al.candidate_lists(pa, pb, kpad, cut, code)[:2]

        def sweep_cols():
            lists["c"] = al.candidate_lists(pb, pa, kpad, cut, code)[:2]

        def build():
            lists["s"] = _lib.sparse_support(*lists["r"], *lists["c"])

        def hits1(**kw):
            gr, ti, _ = al.alignment_counts(e1, e2, True, **kw)
            return al.tie_aware_metrics(gr, ti, [1])[0][0] / n * 100

        res = {"n": n, "d": d, "iters": a.iters, "tau": a.tau, "cut": cut, "noise": a.noise,
               "list_sweep_rows_ms": timed(sweep_rows, a.reps), "list_sweep_cols_ms": timed(sweep_cols, a.reps),
               "support_build_ms": timed(build, a.reps)}
        s = lists["s"]
        res["passes_ms"] = timed(lambda: al.sparse_sinkhorn_potentials(s, a.iters, a.tau), a.reps)
        res["one_row_pass_ms"] = timed(lambda: _lib.sparse_lse(s, False, a.tau), a.reps)
        res["one_col_pass_ms"] = timed(lambda: _lib.sparse_lse(s, True, a.tau), a.reps)
        res["sparse_total_ms"] = timed(lambda: al.sparse_sinkhorn_terms(ops, a.iters, a.tau, cut), a.reps)
        res["entries"] = s.entries()
        res["entries_share"] = res["entries"] / (n * n)
        res["longest_row"] = int((s.row_off[1:] - s.row_off[:-1]).max())
        res["longest_col"] = int((s.col_off[1:] - s.col_off[:-1]).max())
        res["support_mib"] = (res["entries"] * 16 + 2 * (n + 1) * 12) / 2**20
        res["build_temp_mib"] = _lib.sparse_lib().mke_sparse_support_temp_bytes(n, n, cut, cut) / 2**20
        res["plain_hits1"] = hits1()
        res["sparse_hits1"] = hits1(sinkhorn=(a.iters, a.tau, cut))
        if not a.no_dense:
            res["dense_total_ms"] = timed(lambda: al.sinkhorn_terms(*ops, a.iters, a.tau), a.reps)
            res["dense_half_iteration_ms"] = timed(lambda: _lib.align_lse(pa, pb, kpad, a.tau, code), a.reps)
            res["dense_hits1"] = hits1(sinkhorn=(a.iters, a.tau))
            res["dense_over_sparse"] = res["dense_total_ms"] / res["sparse_total_ms"]
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
