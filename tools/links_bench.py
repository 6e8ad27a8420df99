#!/usr/bin/env python3
"""Time of the self-training refresh with and without link accumulation (tools/links_bench.py), and of the link-set edit alone.

    python tools/links_bench.py [--sizes 20000,100000] [--dims 75,256] [--modes off,on] [--windows 7] [--per-window 4] [--tree DIR]

A refresh is what `_ScheduledMultiKE._bootstrap` enqueues: decode (`bootstrap_links`, with a `LinkStore` in mode `on`), link table,
both swaps, ONE read-back.  The arrays have the shape of a schedule's: n candidates a side (KG1 ids [0, n), KG2 ids [n, 2 n)), 5
relation and 3 attribute id-triples per entity, unit rows and a noisy copy.  Two embedding sets alternate from refresh to refresh
(in the second a tenth of the rows of KG2 is turned half-way or fully to a random direction and a fiftieth changes places in
pairs), so that an edit keeps, displaces and expires links as well as re-finding them.  Host clock around windows of
--per-window refreshes (each ends in its read-back); the median, least and largest window per refresh.  `edit_ms`: HIP-event time of `edit_links` alone (the second set's decode against the
first set's links), median of --windows windows of 20 calls.  --tree DIR imports the package from another checkout (a parent commit's, for
mode `off` only: it has no store).  One JSON line per (size, dim, mode)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch


def build(n, dim, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    unit = lambda x: x / x.norm(dim=1, keepdim=True)
    e1 = unit(rnd(n, dim))
    sets = [(e1, e1 + 0.6 / dim ** 0.5 * rnd(n, dim))]      # similarity of a pair ~ 0.86
    e2 = sets[0][1].clone()
    perm = torch.randperm(n, device="cuda", generator=g)
    turned, crossed = perm[:n // 10], perm[n // 10:n // 10 + n // 50 // 2 * 2]
    other = unit(rnd(len(turned), dim))
    half = torch.arange(len(turned), device="cuda") % 2 == 0
    e2[turned] = torch.where(half[:, None], 0.6 * e1[turned] + 0.8 * other, other)     # ~ 0.6: below the threshold, above retain; ~ 0
    e2[crossed] = sets[0][1][crossed.view(-1, 2).flip(1).reshape(-1)]                  # pairs of columns change places: displaced links
    sets.append((e1, e2))
    ints = lambda hi, m: torch.randint(0, hi, (m,), device="cuda", generator=g, dtype=torch.int32)
    cols = {}
    for kind, per, n_pred in (("rel", 5, 500), ("attr", 3, 600)):
        m = 2 * n * per
        h = ints(2 * n, m)
        t = ints(2 * n, m) if kind == "rel" else ints(100_000, m)
        cols[kind] = (h, ints(n_pred, m), t)
    ids1 = torch.arange(n, device="cuda", dtype=torch.int32)
    return sets, cols, ids1, ids1 + n, 2 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,100000")
    ap.add_argument("--dims", default="75,256")
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--per-window", type=int, default=4)
    ap.add_argument("--threshold", type=float, default=0.7)
    ap.add_argument("--retain", type=float, default=0.5)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from multike_amd.base import alignment, bootstrap
    for n in (int(x) for x in a.sizes.split(",")):
        for dim in (int(x) for x in a.dims.split(",")):
            sets, cols, ids1, ids2, n_ent = build(n, dim, n + dim)
            for mode in a.modes.split(","):
                store = bootstrap.LinkStore() if mode == "on" else None
                turn = [0]

                def refresh():
                    e1, e2 = sets[turn[0] % 2]
                    turn[0] += 1
                    kw = dict(store=store, retain=a.retain) if store is not None else {}
                    partner, match, counts, score = bootstrap.bootstrap_links(e1, e2, ids1, ids2, n_ent, a.threshold, 0, scores=True, **kw)
                    rel = bootstrap._swap_launch(cols["rel"], partner, False, None)
                    attr = bootstrap._swap_launch(cols["attr"], partner, True, None)
                    return torch.cat([rel[-1], attr[-1], counts.long()]).cpu().tolist()      # the one read-back
                refresh(), refresh()
                torch.cuda.synchronize()
                per = []
                for _ in range(a.windows):
                    t = time.perf_counter()
                    for _ in range(a.per_window):
                        nums = refresh()
                    torch.cuda.synchronize()
                    per.append((time.perf_counter() - t) * 1e3 / a.per_window)
                out = dict(tree=os.path.relpath(os.path.abspath(a.tree)), candidates=n, dim=dim, mode=mode, windows=a.windows,
                           per_window=a.per_window, refresh_ms=statistics.median(per), refresh_ms_min=min(per), refresh_ms_max=max(per),
                           relation_entries=nums[0], attribute_entries=nums[1], counts=nums[2:])
                if store is not None:
                    if turn[0] % 2 == 0:
                        refresh()                   # the set held is that of the first embedding set, the edit timed is the second's
                    e1, e2 = sets[1]
                    ops = alignment._mutual_operands(e1, e2, "inner", True, 0, None)
                    match, _, row_best = alignment._mutual_decode(ops, a.threshold)
                    best, held = alignment._best_value(row_best), store.held(n)
                    times = []
                    for _ in range(a.windows + 1):
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        for _ in range(20):
                            res = bootstrap.edit_links(held, match, ops, a.retain, best)
                        e.record()
                        e.synchronize()
                        times.append(s.elapsed_time(e) / 20)
                    out["edit_ms"] = statistics.median(times[1:])
                    out["edit_share"] = out["edit_ms"] / out["refresh_ms"]
                    out["edit_counts"] = res[2].cpu().tolist()
                print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)


if __name__ == "__main__":
    main()
