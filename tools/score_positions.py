"""Per-kernel averages, the score launch by its position after the epoch sampler (bins of 10 steps) and the gap from an epoch's
last update launch to the next epoch's first score launch, out of `rocprofv3 --kernel-trace --output-format csv` traces of
bench.py (profiles/r22_neg_codes.md).
python tools/score_positions.py <name>=<kernel_trace.csv> ..."""
import csv, sys, collections
import numpy as np
for arg in sys.argv[1:]:
    t, _, path = arg.partition("=")
    rows = []
    with open(path) as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    print("==", t, len(rows), "dispatches")
    per = collections.defaultdict(list)
    for s, e, k in rows:
        per[k.split("(")[0][:90]].append((e - s) / 1e3)
    for k, v in sorted(per.items(), key=lambda kv: -sum(kv[1]))[:14]:
        print("  %-90s n=%6d avg=%9.2f us total=%9.1f ms" % (k, len(v), np.mean(v), sum(v) / 1e3))
    # position inside an epoch: the sampler launch starts an epoch of the native loop
    pos, bins, inst, gaps = None, collections.defaultdict(list), [], []
    last_upd_end, prev = None, None
    since_sampler = 10 ** 9
    for s, e, k in rows:
        if "k_neg_sample" in k:
            if e - s < 100e3:          # a step's own sampler launch: the Python-driven instrumented pass
                since_sampler = 10 ** 9
                continue
            pos = 0; since_sampler = 0
            boundary_from = last_upd_end
        elif "k_count_refs" in k and "triple" not in k:
            if not (pos == 0 and since_sampler == 0):
                since_sampler = 10 ** 9   # the instrumented pass counts in a launch of its own (the native loop only right after the sampler)
        elif "k_triple_score" in k:
            if pos is not None and since_sampler < 10 ** 9:
                if pos == 0 and boundary_from is not None:
                    gaps.append((s - boundary_from) / 1e3)
                bins[pos // 10].append((e - s) / 1e3); pos += 1
            else:
                inst.append((e - s) / 1e3)
        elif "k_rows_update_multi" in k:
            last_upd_end = e
    for b in sorted(bins):
        if b < 3 or b in (10, 17):
            print("  score launch, steps %3d-%3d after the sampler: n=%5d mean=%.2f us" % (b * 10, b * 10 + 9, len(bins[b]), np.mean(bins[b])))
    steady = [x for b in bins if b >= 10 for x in bins[b]]
    if steady: print("  score launch, steps >= 100: n=%d mean=%.2f us" % (len(steady), np.mean(steady)))
    if inst: print("  score launch, outside the native loop: n=%d mean=%.2f us" % (len(inst), np.mean(inst)))
    if gaps: print("  last update of an epoch -> first score launch of the next: n=%d median=%.1f us min=%.1f max=%.1f" % (len(gaps), np.median(gaps), min(gaps), max(gaps)))
