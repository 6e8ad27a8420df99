#!/usr/bin/env python3
"""Mutual nearest-neighbour sweep on the device (tools/mutual_bench.py): HIP-event times (a warm-up, then the median of --reps
repetitions) of
  1. mke_align_mutual — in its default form (LDS fold of the block's four wavefronts, then one atomic per column and row block)
     and in the three other forms of the column fold (MKE_MUTUAL_FILTER: a load before the atomic; MKE_MUTUAL_NO_LDS_FOLD; both),
  2. mke_align_rank_ex on the same operands: the same sweep without the column fold (an unchanged kernel, same build),
  3. twice (2): the cost of the two-sweep alternative,
at n_a = n_b = 60,000 and 100,000, dim 75 (kpad 80) and dim 256, for the inner product and for inner + re-scoring terms.
One JSON line per (size, dim, mode); the expectation to confirm or refute is (2) <= (1) <= (3).

    python tools/mutual_bench.py [--sizes 60000,100000] [--dims 75,256] [--reps 7]
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
    ap.add_argument("--sizes", default="60000,100000")
    ap.add_argument("--dims", default="75,256")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from multike_amd import _lib
    from multike_amd.base.alignment import prepare_operands
    forms = (("mutual_ms", 0), ("mutual_filter_ms", _lib.MUTUAL_FILTER), ("mutual_no_lds_ms", _lib.MUTUAL_NO_LDS_FOLD),
             ("mutual_no_lds_filter_ms", _lib.MUTUAL_NO_LDS_FOLD | _lib.MUTUAL_FILTER))
    for n in (int(x) for x in a.sizes.split(",")):
        for dim in (int(x) for x in a.dims.split(",")):
            g = torch.Generator(device="cuda").manual_seed(n + dim)
            e2 = torch.randn(n, dim, device="cuda", generator=g)
            e1 = e2 + 0.7 * torch.randn(n, dim, device="cuda", generator=g)
            ap_, bp, kpad, code, _, _ = prepare_operands(e1, e2, "inner", True, "cuda")
            del e1, e2
            r_t = 0.1 * torch.rand(n, device="cuda", generator=g)
            r_s = 0.1 * torch.rand(n, device="cuda", generator=g)
            rank, ties, best = (torch.zeros(n, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.int64))
            out = (torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda"))

            def mutual(terms, flags):
                # the words are zeroed inside the timed region: a filter that found the last repetition's words would skip everything
                out[0].zero_()
                out[1].zero_()
                _lib.align_mutual(ap_, bp, kpad, code, None, None, *terms, flags=flags, out=out)

            for mode, terms in (("inner", (None, None)), ("inner+terms", (r_t, r_s))):
                res = {"n": n, "dim": dim, "kpad": kpad, "mode": mode}
                res["rank_ex_ms"] = timed(lambda: _lib.align_rank_ex(ap_, bp, kpad, rank, ties, best, code, None, None, *terms), a.reps)
                res["two_sweeps_ms"] = 2 * res["rank_ex_ms"]
                for name, flags in forms:
                    res[name] = timed(lambda: mutual(terms, flags), a.reps)
                res["zero_words_ms"] = timed(lambda: (out[0].zero_(), out[1].zero_()), a.reps)
                res["mutual_over_rank_ex"] = res["mutual_ms"] / res["rank_ex_ms"]
                res["between"] = res["rank_ex_ms"] <= res["mutual_ms"] <= res["two_sweeps_ms"]
                print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
