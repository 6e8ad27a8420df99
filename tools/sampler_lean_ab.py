"""The lean form of the fast sampler kernels (EXPERIMENTS R25.1) switched at run time inside ONE process, on bench.py's own
workload object as tools/sampler_codes_ab.py does: the same allocations for both variants.  920-step windows bracketed as bench.py
brackets them, each 20 steps into an epoch.  Variants: off = the fast form's kernels as they were (`sampler_lean` 0); on = the
lean form (wave-uniform side, 32-bit offsets, its own prefilter, strided grid).  The negatives are the same bit for bit.
The bar (profiles/r08_epoch_boundary.md): median(on) below median(off) by more than three times the larger min-max spread of the two.
python tools/sampler_lean_ab.py [rounds]"""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import bench
from multike_amd import _lib
cfg = dict(bench.CONFIGS["c2"])
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
w = bench.FusedWorkload(cfg)
variants = {"off": dict(sampler_lean=0), "on": dict(sampler_lean=1)}
def set_variant(v):
    torch.cuda.synchronize()
    for k, x in variants[v].items():
        _lib.set_option(k, x)
n = w.n_steps_epoch
i = 0
w.run_steps(0, n); i = n
w.run_steps(i, i + 20); i += 20
res = {v: [] for v in variants}
for rep in range(reps):
    for v in variants:
        set_variant(v)
        k = 20 + (n - (i + 20) % n) % n + 20
        w.run_steps(i, i + k); i += k
        dt = w.timed(i, 920); i += 920
        res[v].append(dt * 1e3)
        print(rep, v, "%.3f ms" % (dt * 1e3), flush=True)
set_variant("on")
out = {v: {"min": min(x), "median": float(np.median(x)), "max": max(x), "all": x} for v, x in res.items()}
spread = max(o["max"] - o["min"] for o in out.values())
out["gain_ms"] = out["off"]["median"] - out["on"]["median"]
out["bar_ms"] = 3 * spread
out["passed"] = bool(out["gain_ms"] > out["bar_ms"])
print(json.dumps(out))
