#!/usr/bin/env python3
"""Record tests/golden/sinkhorn_parent_counters.npz: what `alignment_counts` / `greedy_alignment` WITH DEFAULTS return on the
first case of sinkhorn_golden.npz, plain and with CSLS k = 10 — run on a GPU from a checkout of the commit BEFORE the Sinkhorn
re-scoring was added, so that tests/test_sinkhorn_eval_gpu.py can hold every later commit to the same counters bit for bit.

    python tests/golden/record_parent_counters.py --root <checkout of the parent commit, built> [--out FILE]

--root is the tree whose `multike_amd` package is imported (default: the tree this script lies in)."""
import argparse
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TOP_K = [1, 5, 10, 50]
CASE, CSLS_K = "inner_100", 10


def record():
    """{key: array} from whichever multike_amd is importable."""
    from multike_amd.base.alignment import alignment_counts, greedy_alignment
    g = np.load(os.path.join(HERE, "sinkhorn_golden.npz"))
    e1, e2 = g[CASE + "/e1"], g[CASE + "/e2"]
    out = {}
    for tag, k in (("plain", 0), ("csls", CSLS_K)):
        greater, ties, best = alignment_counts(e1, e2, normalize=True, csls_k=k)
        with contextlib.redirect_stdout(io.StringIO()):
            pairs, hits1, mr, mrr = greedy_alignment(e1, e2, TOP_K, 1, "inner", True, k, True)
        out.update({tag + "/greater": greater.cpu().numpy(), tag + "/ties": ties.cpu().numpy(), tag + "/best": best.cpu().numpy(),
                    tag + "/pairs": np.array(sorted(pairs), dtype=np.int64),
                    tag + "/metrics": np.array([hits1, mr, mrr], dtype=np.float64)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)))
    ap.add_argument("--out", default=os.path.join(HERE, "sinkhorn_parent_counters.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import multike_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(multike_amd.__file__))) == os.path.abspath(a.root), multike_amd.__file__
    np.savez_compressed(a.out, **record())
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes) from {a.root}")


if __name__ == "__main__":
    main()
