"""k-NN refresh with and without a capped table, time and peak memory in one process:
    [REPS=5] [PART=r,G] [KEYED=1,0] [Z=3] [NSAMP=65536] python tools/capped_knn_bench.py [n] [dim] [k] [cap,cap,...]
(cap 0 = the uncapped call; default 0,256,2048).  A tree whose neighbour_table has no `cap` yet (the parent of the capped refresh)
runs the uncapped call only, so the same script gives the line the capped calls are compared against.  Each call is made `REPS`
times after one warm-up call; the median and the spread are printed, and the peak of torch's allocator over one call (operands
included).  KEYED = a comma list of the paths of a capped call to compare — 1 the keyed (matrix-free) selection, 0 without it,
auto the call's own rule (the default) — run ALTERNATING, one warm-up call each, so that both see the same machine; Z and NSAMP
override the keyed path's `keyed_params`, and the line of a keyed call carries its `stats` (rows redone, by status)."""
import inspect, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from multike_amd.base.batch import neighbour_table

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 75
k = int(sys.argv[3]) if len(sys.argv) > 3 else int(0.02 * n)
caps = [int(x) for x in sys.argv[4].split(",")] if len(sys.argv) > 4 else [0, 256, 2048]
REPS = int(os.environ.get("REPS", "5"))
PART = tuple(int(x) for x in os.environ["PART"].split(",")) if os.environ.get("PART") else None   # "r,G": one slice of the rows only
has_cap = "cap" in inspect.signature(neighbour_table).parameters
has_keyed = "keyed" in inspect.signature(neighbour_table).parameters
MODES = [{"1": True, "0": False, "auto": None}[x] for x in os.environ.get("KEYED", "auto").split(",")] if has_keyed else [None]
PARAMS = {a: f(os.environ[b]) for a, b, f in (("z", "Z", float), ("n_samp", "NSAMP", int)) if os.environ.get(b)}
g = torch.Generator(device="cuda"); g.manual_seed(0)
centers = torch.randn(200, d, device="cuda", generator=g)
e = centers[torch.randint(0, 200, (n,), device="cuda", generator=g)] + 0.8 * torch.randn(n, d, device="cuda", generator=g)
e = torch.nn.functional.normalize(e, dim=1)
del centers
ids = np.arange(n)
for cap in caps:
    if cap and not has_cap:
        print(json.dumps({"cap": cap, "skipped": "this tree's neighbour_table takes no cap"}))
        continue
    modes = MODES if cap else [None]
    ms, peak, stats, width = {m: [] for m in modes}, {m: 0 for m in modes}, {m: {} for m in modes}, 0
    for it in range(REPS + 1):
        for mode in modes:                                # alternating: warm-up call of every path, then REPS rounds
            kw = {"cap": cap, "seed": 1} if cap else {}
            if PART:
                kw["part"] = PART
            if has_keyed and cap:
                kw.update(keyed=mode, stats=stats[mode], **({"keyed_params": PARAMS} if PARAMS else {}))
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); t0 = time.perf_counter()
            table, valid = neighbour_table(e, ids, k, n, **kw)[:2]
            torch.cuda.synchronize()
            if it:
                ms[mode].append((time.perf_counter() - t0) * 1e3)
            peak[mode] = max(peak[mode], torch.cuda.max_memory_allocated())
            width = int(table.shape[1])
            del table, valid
    for mode in modes:
        t = np.sort(np.asarray(ms[mode]))
        line = {"n": n, "dim": d, "k": k, "cap": cap or None, "part": PART, "table_width": width, "reps": REPS,
                "ms_median": round(float(np.median(t)), 2), "ms_min": round(float(t[0]), 2), "ms_max": round(float(t[-1]), 2),
                "peak_MiB": round(peak[mode] / 2**20, 1)}
        if has_keyed and cap:
            line.update(keyed={True: 1, False: 0, None: "auto"}[mode], keyed_params=PARAMS or None, stats=stats[mode] or None)
        print(json.dumps(line), flush=True)
