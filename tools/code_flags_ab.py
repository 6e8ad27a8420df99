"""`code_flags` (EXPERIMENTS R28.1) switched at run time inside ONE process, on bench.py's own workload object as
tools/neg_codes_ab.py does: the same allocations for both variants.  920-step windows bracketed as bench.py brackets them, each
20 steps into an epoch.  off = entity touched flags stored by the score launch and scanned by the update launch, on = no entity
flags, the update launch reads the step's row of the bake's bitmap and the step's positives.
python tools/code_flags_ab.py [rounds]"""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import bench
from multike_amd import _lib
cfg = dict(bench.CONFIGS["c2"])
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
w = bench.FusedWorkload(cfg)
variants = {"off": 0, "on": 1}
def set_variant(v):
    torch.cuda.synchronize()
    _lib.set_option("code_flags", variants[v])
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
spread = max(out[v]["max"] - out[v]["min"] for v in out)
out["gain_ms"] = out["off"]["median"] - out["on"]["median"]
out["bar_ms"] = 3 * spread
out["every_on_below_every_off"] = out["on"]["max"] < out["off"]["min"]
print(json.dumps(out))
