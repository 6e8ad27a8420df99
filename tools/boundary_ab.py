"""The three parts of the epoch boundary (EXPERIMENTS R8.1) switched at run time inside ONE process: the same allocations for every
variant, so the per-process placement differences (R5.10) do not sit between them.  Times 920-step windows of bench.py's fused
workload exactly as bench.py brackets them.  Variants: 0 = none (the boundary as it was: exact probe for every candidate, the
torch gather chain, permutations drawn in line), F = known-triple prefilter, G = mke_epoch_positives, P = permutations drawn one
epoch ahead; FG, FGP; G and P alone.
python tools/boundary_ab.py [c2|c5] [rounds]"""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import bench
from multike_amd import _lib
cfg = dict(bench.CONFIGS[sys.argv[1] if len(sys.argv) > 1 else "c2"])
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
w = bench.FusedWorkload(cfg)
bat = w.bat
one = [torch.as_tensor(w.kgs.triples[k][:1].astype(np.int32), device="cuda") for k in (0, 1)]

def set_variant(v):
    torch.cuda.synchronize()
    for k, sd in enumerate((bat.side1, bat.side2)):
        keys = sd.known.keys
        if "F" in v:
            t = one[k]
            _lib.tripleset_build(t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous(), keys)  # (re)creates the filter from the table
            assert _lib.tripleset_filter_bytes(keys) > 0
        else:
            _lib.tripleset_forget(keys)
            assert _lib.tripleset_filter_bytes(keys) == 0
    bat._native = "G" in v
    if bat._native and bat.t1.data_ptr() in (bat._spare_lists[0].data_ptr(),):
        bat._spare_lists = (torch.empty_like(bat.t1), torch.empty_like(bat.t2))
    bat._prefetch = "P" in v
    bat._perm_stream = None
    torch.cuda.synchronize()

n = w.n_steps_epoch
i = 0
w.run_steps(0, n); i = n
w.run_steps(i, i + 20); i += 20
variants = ["0", "F", "FG", "FGP", "G", "P"]
res = {v: [] for v in variants}
for rep in range(reps):
    for v in variants:
        set_variant(v)
        w.run_steps(i, i + 20 + (n - (i + 20) % n) % n + 20); i += 20 + (n - (i + 20) % n) % n + 20   # settle: to 20 steps into an epoch
        dt = w.timed(i, 920); i += 920
        res[v].append(dt * 1e3)
        print(rep, v, "%.3f ms" % (dt * 1e3), flush=True)
print(json.dumps({v: {"min": min(x), "median": float(np.median(x)), "max": max(x)} for v, x in res.items()}))
